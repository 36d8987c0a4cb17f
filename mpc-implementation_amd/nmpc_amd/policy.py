"""Applying the plan's feedback policy between two solves.

:meth:`nmpc_amd.nlpsol.Solver.policy_device` returns, per scenario, the stage gains K_k, the
feedforward kff_k per parameter direction and the plan's states X*_k; :func:`apply` evaluates

    u_k(x, c) = u*_k + K_k (x - X*_k) + sum_d kff_k^(d) c_d

with torch ops on the caller's stream: nothing is copied to the host.  :func:`rollout` runs that
policy, clamped, on the nonlinear plant for many disturbance samples per scenario in one launch
(``Solver.policy_rollout_device``): what it costs and whether it keeps the rows.  :func:`covariance`
gives what those rollouts estimate in closed form, the state covariance around the plan and the
standard deviation of every row and control (``Solver.policy_covariance_device``),
:func:`covariance_grad` its reverse sweep (``Solver.policy_covariance_adjoint_device``),
:func:`tighten` moves the bounds of the next solve inwards by a multiple of them, and
:func:`expected_cost` gives the policy's expected cost and its variance to second order
(``Solver.policy_value_device``)."""
from __future__ import annotations


def apply(pol: dict, sol: dict, k: int, x_meas, c=None, lbx=None, ubx=None):
    """The policy's control at stage ``k`` for the measured states ``x_meas`` (B, nx).

    ``pol`` is the dict of ``Solver.policy_device``; ``sol["x"]`` (B, nw) holds the plan's
    controls.  ``c`` (B, nd) or (nd,) are the coefficients of the parameter move along the
    directions the policy was formed for (None: no move).  ``lbx`` / ``ubx`` ((nw,) or (B, nw)),
    when given, clamp the result to stage k's control bounds.  Returns (B, nu); a scenario whose
    ``info`` is not 0 gets a NaN row."""
    import torch

    K, X = pol["K"], pol["X"]
    nu = K.shape[2]
    u = sol["x"][:, k * nu:(k + 1) * nu] + torch.einsum("bij,bj->bi", K[:, k], x_meas - X[:, k])
    if c is not None:
        kff = pol["kff"]
        if kff is None:
            raise ValueError("the policy holds no feedforward: it was formed without directions")
        cc = c if c.dim() == 2 else c.unsqueeze(0).expand(kff.shape[0], -1)
        u = u + torch.einsum("bdi,bd->bi", kff[:, :, k], cc)

    def stage(v):
        return v[..., k * nu:(k + 1) * nu]

    if lbx is not None:
        u = torch.maximum(u, stage(lbx))
    if ubx is not None:
        u = torch.minimum(u, stage(ubx))
    bad = (pol["info"] != 0).unsqueeze(1)
    return torch.where(bad, torch.full_like(u, float("nan")), u)


def rollout(solver, pol: dict, sol: dict, p, e0, w=None, c=None, lbx=None, ubx=None, lbg=None, ubg=None,
            feedback: bool = True, out: dict | None = None, want=("J", "viol", "nsat"), stream=None):
    """M disturbance rollouts per scenario of the clamped policy on the nonlinear plant, in one
    launch (``Solver.policy_rollout_device``): what the policy costs and whether it keeps the rows
    when the state starts ``e0`` (B, M, nx) away from the plan and is pushed by ``w`` (B, M, N, nx)
    at every stage (None: no process disturbance).

    ``pol`` is the dict of ``Solver.policy_device``, ``sol["x"]`` (B, nw) the plan's controls and
    ``p`` (B, np) the parameters the plant runs with -- after a parameter move along the policy's
    directions the moved ones, with ``c`` (B, nd) or (nd,) the move's coefficients: the nominal
    controls are then ubar = u* + sum_d kff^(d) c_d.  ``feedback=False`` replays ubar open loop
    (no gains), the baseline the feedback is measured against.  ``lbx`` / ``ubx`` clamp the
    controls, ``lbg`` / ``ubg`` are the rows' bounds for ``viol``.  Returns the dict of
    ``Solver.policy_rollout_device``: ``J``, ``viol``, ``nsat`` (B, M) and, when asked for in
    ``want`` or preallocated in ``out``, ``X`` (B, M, N+1, nx) and ``U`` (B, M, N, nu).  A scenario
    whose ``info`` is not 0 has NaN gains and plan, hence NaN J and viol.  Nothing is copied to the
    host and nothing synchronises."""
    import torch

    ubar = sol["x"]
    if c is not None:
        kff = pol["kff"]
        if kff is None:
            raise ValueError("the policy holds no feedforward: it was formed without directions")
        cc = c if c.dim() == 2 else c.unsqueeze(0).expand(kff.shape[0], -1)
        ubar = ubar + torch.einsum("bdn,bd->bn", kff.reshape(kff.shape[0], kff.shape[1], -1), cc)
    raw = pol["raw"]
    return solver.policy_rollout_device(p, ubar.contiguous(), raw["X"], raw["K"] if feedback else None, e0, w=w,
                                        lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg, out=out, want=want, stream=stream)


def rollout_grad(solver, pol: dict, sol: dict, p, X, Jb=None, Xb=None, Ub=None, c=None, lbx=None, ubx=None,
                 feedback: bool = True, out: dict | None = None, want=("ubar_bar", "p_bar"), stream=None):
    """The gradient of a loss on :func:`rollout`'s samples, in one launch
    (``Solver.policy_rollout_adjoint_device``): with ``X`` (B, M, N+1, nx) the trajectories that
    :func:`rollout` returned for the same ``pol``, ``sol``, ``p``, ``c``, bounds and ``feedback``,
    and seeds ``Jb`` (B, M) on J, ``Xb`` (B, M, N+1, nx) on X and ``Ub`` (B, M, N, nu) on the applied
    controls (each may be None, one at least is given), the derivative of
    sum_s (Jb_s J_s + <Xb_s, X_s> + <Ub_s, U_s>) per scenario with respect to the nominal controls
    (``ubar_bar`` (B, nw)), the gains (``K_bar`` (B, N, nx, nu), the raw column-major blocks), the
    plan's states (``Xbar_bar``), the parameters (``p_bar``) and each sample's disturbances
    (``e0_bar``, ``w_bar``), as asked for in ``want`` or preallocated in ``out``.  With ``c`` given,
    ubar = u* + sum_d kff^(d) c_d, and the dict also holds ``c_bar`` (B, nd) = <kff^(d), ubar_bar>
    (``ubar_bar`` is then formed whether asked for or not).  Jb = 1 / M gives the gradient of the
    mean sampled cost.  Nothing is copied to the host and nothing synchronises."""
    import torch

    ubar = sol["x"]
    kff = None
    if c is not None:
        kff = pol["kff"]
        if kff is None:
            raise ValueError("the policy holds no feedforward: it was formed without directions")
        cc = c if c.dim() == 2 else c.unsqueeze(0).expand(kff.shape[0], -1)
        ubar = ubar + torch.einsum("bdn,bd->bn", kff.reshape(kff.shape[0], kff.shape[1], -1), cc)
        if "ubar_bar" not in want:
            want = tuple(want) + ("ubar_bar",)
    raw = pol["raw"]
    res = solver.policy_rollout_adjoint_device(p, ubar.contiguous(), raw["X"], raw["K"] if feedback else None, X,
                                               Jb=Jb, Xb=Xb, Ub=Ub, lbx=lbx, ubx=ubx, out=out, want=want,
                                               stream=stream)
    if kff is not None:
        res["c_bar"] = torch.einsum("bdn,bn->bd", kff.reshape(kff.shape[0], kff.shape[1], -1), res["ubar_bar"])
    return res


def covariance(solver, pol: dict, sol: dict, p, S0, W=None, obs_var=None, c=None, feedback: bool = True,
               out: dict | None = None, want=("sigma_g", "sigma_u"), stream=None):
    """The state covariance around the plan under the policy, to first order, and the standard
    deviations of every row and every control, in one launch (``Solver.policy_covariance_device``):
    the number :func:`rollout` estimates by sampling, without the sampling noise.  ``S0`` (B, nc, nx,
    nx) or (nc, nx, nx) holds one covariance of the initial state per case, ``W`` likewise the process
    noise added at every stage (None: none), ``obs_var`` (B, n_obs) or (n_obs,) the isotropic
    variance of each obstacle's centre.  ``pol``, ``sol``, ``p``, ``c`` and ``feedback`` are
    :func:`rollout`'s: the nominal controls are ubar = u* + sum_d kff^(d) c_d, and ``feedback=False``
    propagates the open loop.  Returns the dict of ``Solver.policy_covariance_device``: ``sigma_g``
    (B, nc, N+1, m), ``sigma_u`` (B, nc, N, nu) and, when asked for, ``Sigma`` (B, nc, N+1, nx, nx).
    The gains are used as they are: where the plan holds a control on its bound, zero its row of
    ``pol["raw"]["K"]`` first if the clamp is to count.  Nothing is copied to the host and nothing
    synchronises."""
    import torch

    ubar = sol["x"]
    if c is not None:
        kff = pol["kff"]
        if kff is None:
            raise ValueError("the policy holds no feedforward: it was formed without directions")
        cc = c if c.dim() == 2 else c.unsqueeze(0).expand(kff.shape[0], -1)
        ubar = ubar + torch.einsum("bdn,bd->bn", kff.reshape(kff.shape[0], kff.shape[1], -1), cc)
    raw = pol["raw"]
    return solver.policy_covariance_device(p, ubar.contiguous(), raw["X"], raw["K"] if feedback else None, S0, W=W,
                                           obs_var=obs_var, out=out, want=want, stream=stream)


def expected_cost(solver, pol: dict, sol: dict, p, S0, W=None, feedback: bool = True, out: dict | None = None,
                  want=("J", "dJ", "varJ"), stream=None):
    """The expected cost of the unclamped policy under an uncertain initial state and process noise, to
    second order, in one launch (``Solver.policy_value_device``): the number the mean of
    :func:`rollout`'s sampled J estimates, without the sampling noise.  ``S0`` (B, nc, nx, nx) or (nc,
    nx, nx) holds one covariance of the initial state per case and ``W`` likewise the process noise
    added at every stage (None: none), as :func:`covariance` takes them; ``feedback=False`` expands the
    open loop.  Returns the dict of ``Solver.policy_value_device``: ``J`` (B,) the plan's own cost,
    ``dJ`` (B, nc) the second-order shift of its mean, ``varJ`` (B, nc) its variance to first order
    and, when asked for in ``want`` or preallocated in ``out``, ``lam`` (B, N+1, nx) and ``P`` (B, N+1,
    nx, nx), the gradient and Hessian of the cost-to-go at every stage; with ``J`` and ``dJ`` both
    there, also ``EJ`` (B, nc) = J + dJ.
    The expansion is taken at ``pol``'s states and ``sol``'s controls, which are the closed loop's own
    undisturbed trajectory.  There is no parameter move ``c`` here: after one the plan's states are no
    longer the trajectory of the moved controls, and the first-order terms this expansion leaves out
    would not vanish.  Nothing is copied to the host and nothing synchronises."""
    raw = pol["raw"]
    res = solver.policy_value_device(p, sol["x"].contiguous(), raw["X"], raw["K"] if feedback else None, S0=S0, W=W,
                                     out=out, want=want, stream=stream)
    if res.get("J") is not None and res.get("dJ") is not None:
        res["EJ"] = res["J"].unsqueeze(1) + res["dJ"]
    return res


def var_seed(sigma, sigma_b):
    """The seed on a variance for the seed ``sigma_b`` on its standard deviation sigma = sqrt(max(var, 0)):
    sigma_b / (2 sigma) where sigma > 0, 0 where sigma == 0 (the maximum's flat side), NaN where sigma is
    NaN.  Torch ops only."""
    import torch

    safe = torch.where(sigma > 0, sigma, torch.ones_like(sigma))
    return torch.where(sigma > 0, sigma_b / (2.0 * safe), torch.where(sigma != sigma, sigma, torch.zeros_like(sigma)))


def covariance_grad(solver, pol: dict, sol: dict, p, cov: dict, Sigma_b=None, sigma_u_b=None, sigma_g_b=None, c=None,
                    feedback: bool = True, out: dict | None = None,
                    want=("S0_bar", "K_bar", "ubar_bar", "Xbar_bar", "p_bar"), stream=None):
    """The gradient of a loss on :func:`covariance`'s result, in one launch
    (``Solver.policy_covariance_adjoint_device``): ``cov`` is the dict :func:`covariance` returned for
    the same ``pol``, ``sol``, ``p``, ``c`` and ``feedback`` and must hold ``Sigma``; the seeds
    ``Sigma_b`` (B, nc, N+1, nx, nx), ``sigma_u_b`` (B, nc, N, nu) and ``sigma_g_b`` (B, nc, N+1, m) are on
    Sigma and on the STANDARD DEVIATIONS (each may be None, one at least is given; ``cov`` must hold the
    deviations that are seeded).  They are turned into seeds on the variances with :func:`var_seed`.
    Returns the dict of ``Solver.policy_covariance_adjoint_device`` with the outputs asked for in
    ``want`` or preallocated in ``out``, each per (scenario, case).  With ``c`` given,
    ubar = u* + sum_d kff^(d) c_d, and the dict also holds ``c_bar`` (B, nc, nd) = <kff^(d), ubar_bar>
    (``ubar_bar`` is then formed whether asked for or not).  With ``feedback=False`` the gains are not
    read, ``sigma_u_b`` contributes nothing and ``K_bar`` is left out.  Nothing is copied to the host
    and nothing synchronises."""
    import torch

    if cov.get("Sigma") is None:
        raise ValueError("cov holds no Sigma: ask policy.covariance for it (want=(..., 'Sigma'))")
    ubar = sol["x"]
    kff = None
    if c is not None:
        kff = pol["kff"]
        if kff is None:
            raise ValueError("the policy holds no feedforward: it was formed without directions")
        cc = c if c.dim() == 2 else c.unsqueeze(0).expand(kff.shape[0], -1)
        ubar = ubar + torch.einsum("bdn,bd->bn", kff.reshape(kff.shape[0], kff.shape[1], -1), cc)
        if "ubar_bar" not in want:
            want = tuple(want) + ("ubar_bar",)
    if not feedback:
        want = tuple(k for k in want if k != "K_bar")
    vu = None if (sigma_u_b is None or not feedback) else var_seed(cov["sigma_u"], sigma_u_b).contiguous()
    vg = None if sigma_g_b is None else var_seed(cov["sigma_g"], sigma_g_b).contiguous()
    raw = pol["raw"]
    res = solver.policy_covariance_adjoint_device(p, ubar.contiguous(), raw["X"], raw["K"] if feedback else None,
                                                  cov["Sigma"], Sigma_bar=Sigma_b, var_u_bar=vu, var_g_bar=vg, out=out,
                                                  want=want, stream=stream)
    if kff is not None:
        res["c_bar"] = torch.einsum("bdn,bcn->bcd", kff.reshape(kff.shape[0], kff.shape[1], -1), res["ubar_bar"])
    return res


BOUND_INF = 1e19  # a bound at or beyond it is absent (IPOPT's nlp_lower / upper_bound_inf)


def tighten(lbx, ubx, lbg, ubg, cov: dict, kappa, case: int = 0):
    """The four bounds moved inwards by ``kappa`` standard deviations of case ``case`` of
    :func:`covariance`'s result (``sigma_u`` for lbx / ubx, ``sigma_g`` for lbg / ubg): the bounds of
    the next solve.  Each bound is (n,) or (B, n); the four results are (B, n).  A bound with
    |b| >= 1e19 is absent and stays as it is; a fixed variable (lbx == ubx) and an equality row
    (lbg == ubg) stay untouched; a pair that would cross -- the back-offs exceed the room between the
    bounds -- collapses to its midpoint, so lower <= upper always holds (such a pair then fixes the
    variable or the row: the room was smaller than the uncertainty asked for).  Torch ops only, on the
    tensors' device and stream."""
    import torch

    def pair(lo, hi, sigma):
        B = sigma.shape[0]
        back = kappa * sigma[:, case].reshape(B, -1)
        lo = lo.expand(B, -1) if lo.dim() == 2 else lo.unsqueeze(0).expand(B, -1)
        hi = hi.expand(B, -1) if hi.dim() == 2 else hi.unsqueeze(0).expand(B, -1)
        free = lo != hi
        tl = torch.where(free & (lo.abs() < BOUND_INF), lo + back, lo)
        th = torch.where(free & (hi.abs() < BOUND_INF), hi - back, hi)
        mid = 0.5 * (lo + hi)
        cross = tl > th
        return torch.where(cross, mid, tl), torch.where(cross, mid, th)

    nlx, nux = pair(lbx, ubx, cov["sigma_u"])
    nlg, nug = pair(lbg, ubg, cov["sigma_g"])
    return nlx, nux, nlg, nug
