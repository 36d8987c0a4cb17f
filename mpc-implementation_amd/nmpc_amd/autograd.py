"""``torch.autograd`` over the batched solve: the NMPC law as a differentiable layer.

    x, X = nmpc_amd.autograd.solve(solver, p, lbx, ubx, lbg, ubg)
    loss(x, X).backward()          # p.grad: d loss / d p, every entry of p at once

Forward is :meth:`Solver.solve_device`; backward is :meth:`Solver.sensitivity_adjoint` (one KKT
solve with one right-hand side and one transposed product per scenario, whatever np is), or with
``backward="device"`` one :meth:`Solver.sensitivity_adjoint_device` launch that reads nothing
back.  Forward mode (``torch.autograd.forward_ad`` dual tensors on p) gives the tangents of x and
X: one :meth:`Solver.sensitivity_device` launch with ``backward="device"``,
:meth:`Solver.sensitivity_fused` otherwise.  This module holds no mathematics of its own.  torch
is imported lazily, as the device methods do.
"""
from __future__ import annotations

import functools

import numpy as np

_SUCCESS = (0, 1)


@functools.lru_cache(maxsize=None)
def _function():
    import torch

    class _Solve(torch.autograd.Function):
        @staticmethod
        def forward(ctx, p, solver, lbx, ubx, lbg, ubg, x0, device):
            assert p.dtype == torch.float64 and p.is_cuda and p.dim() == 2 and p.shape[1] == solver.np, tuple(p.shape)
            B = p.shape[0]
            f64 = dict(dtype=torch.float64, device=p.device)
            pd = p.detach().contiguous()
            bounds = [np.asarray(v, dtype=np.float64) for v in (lbx, ubx, lbg, ubg)]
            dev = [torch.tensor(np.ascontiguousarray(v.T if v.ndim == 2 else v), **f64) for v in bounds]
            w0 = torch.zeros(B, solver.nw, **f64) if x0 is None else x0.detach().contiguous()
            out = {"x": torch.empty(B, solver.nw, **f64), "g": torch.empty(B, solver.ng, **f64),
                   "lam_x": torch.empty(B, solver.nw, **f64), "lam_g": torch.empty(B, solver.ng, **f64),
                   "X": torch.empty(B, solver.nX, **f64),
                   "status": torch.empty(B, dtype=torch.int32, device=p.device)}
            solver.solve_device(w0, *dev, pd, out)
            ctx.set_materialize_grads(False)  # an output the loss does not read seeds nothing
            ctx.solver, ctx.bounds, ctx.device = solver, bounds, device
            if device:  # everything stays where it is: no copy, no synchronisation
                ctx.sol = {k: out[k].detach() for k in ("x", "g", "lam_x", "lam_g")}
                ctx.p, ctx.dev, ctx.status = pd, dev, out["status"]
                return out["x"], out["X"]
            # the solution as sensitivity_adjoint takes it: columns per scenario, on the host
            ctx.sol = {k: out[k].cpu().numpy().T for k in ("x", "g", "lam_x", "lam_g")}
            ctx.p = pd.cpu().numpy().T
            ctx.status = out["status"].cpu().numpy()
            return out["x"], out["X"]

        @staticmethod
        def backward(ctx, x_bar, X_bar):
            if ctx.device:
                ref = x_bar if x_bar is not None else X_bar
                B, s = ctx.p.shape[0], ctx.solver
                seeds = {k: None if t is None else t.detach().to(torch.float64).contiguous().reshape(B, 1, n)
                         for k, t, n in (("x_bar", x_bar, s.nw), ("X_bar", X_bar, s.nX))}
                o = {"pbar": torch.empty(B, 1, s.np, dtype=torch.float64, device=ref.device),
                     "info": torch.empty(B, dtype=torch.int32, device=ref.device)}
                s.sensitivity_adjoint_device(ctx.sol, *ctx.dev, ctx.p, o, **seeds)
                ok = (o["info"] == 0) & ((ctx.status == 0) | (ctx.status == 1))
                g = torch.where(ok[:, None], o["pbar"][:, 0, :], torch.full_like(o["pbar"][:, 0, :], float("nan")))
                return (g,) + (None,) * 7

            def seed(t):  # (B, n) -> (n, 1, B)
                return None if t is None else np.ascontiguousarray(t.detach().cpu().numpy().T[:, None, :])

            r = ctx.solver.sensitivity_adjoint(ctx.sol, *ctx.bounds, ctx.p, x_bar=seed(x_bar), X_bar=seed(X_bar))
            g = np.ascontiguousarray(r["pbar"][:, 0, :].T)  # (B, np); NaN rows where info != 0
            g[~np.isin(ctx.status, _SUCCESS)] = np.nan
            ref = x_bar if x_bar is not None else X_bar
            return (torch.tensor(g, dtype=torch.float64, device=ref.device),) + (None,) * 7

        @staticmethod
        def jvp(ctx, p_t, *_):
            if p_t is None:
                return None, None
            B, s = ctx.p.shape[0] if ctx.device else ctx.p.shape[1], ctx.solver
            f64 = dict(dtype=torch.float64, device=p_t.device)
            if ctx.device:
                dp = p_t.detach().to(torch.float64).contiguous().reshape(B, 1, s.np)
                o = {"dx": torch.empty(B, 1, s.nw, **f64), "dX": torch.empty(B, 1, s.nX, **f64),
                     "info": torch.empty(B, dtype=torch.int32, device=p_t.device)}
                s.sensitivity_device(ctx.sol, *ctx.dev, ctx.p, dp, o)
                ok = (o["info"] == 0) & ((ctx.status == 0) | (ctx.status == 1))
                nan = float("nan")
                return tuple(torch.where(ok[:, None], o[k][:, 0, :], torch.full_like(o[k][:, 0, :], nan))
                             for k in ("dx", "dX"))
            dp = np.ascontiguousarray(p_t.detach().cpu().numpy().T[:, None, :])  # (np, 1, B)
            r = ctx.solver.sensitivity_fused(ctx.sol, *ctx.bounds, ctx.p, dp)
            bad = ~np.isin(ctx.status, _SUCCESS) | (r["info"] != 0)
            res = []
            for k in ("dx", "dX"):
                t = np.ascontiguousarray(r[k][:, 0, :].T)  # (B, n)
                t[bad] = np.nan
                res.append(torch.tensor(t, **f64))
            return tuple(res)

    return _Solve


@functools.lru_cache(maxsize=None)
def _rollout_function():
    import torch

    class _Rollout(torch.autograd.Function):
        @staticmethod
        def forward(ctx, solver, p, ubar, Xbar, K, e0, w, lbx, ubx):
            det = [None if t is None else t.detach().contiguous() for t in (p, ubar, Xbar, K, e0, w, lbx, ubx)]
            pd, ud, Xd, Kd, ed, wd, lo, hi = det
            _, nu, nx = solver._policy_dims()
            ctx.k_view = Kd is not None and tuple(Kd.shape[-2:]) == (nu, nx)
            if ctx.k_view:  # policy_device's view (…, nu, nx): to the kernel's column-major blocks
                Kd = Kd.transpose(-1, -2).contiguous()
            r = solver.policy_rollout_device(pd, ud, Xd, Kd, ed, w=wd, lbx=lo, ubx=hi, want=("J", "X", "U"))
            ctx.set_materialize_grads(False)  # an output the loss does not read seeds nothing
            ctx.solver, ctx.ins, ctx.X = solver, (pd, ud, Xd, Kd, lo, hi), r["X"]
            ctx.has_w = wd is not None
            return r["J"], r["X"], r["U"]

        @staticmethod
        def backward(ctx, Jb, Xb, Ub):
            s = ctx.solver
            pd, ud, Xd, Kd, lo, hi = ctx.ins
            if Jb is None and Xb is None and Ub is None:
                return (None,) * 9
            need = ctx.needs_input_grad  # (solver, p, ubar, Xbar, K, e0, w, lbx, ubx)
            names = ((1, "p_bar"), (2, "ubar_bar"), (3, "Xbar_bar"), (4, "K_bar"), (5, "e0_bar"), (6, "w_bar"))
            want = tuple(n for i, n in names if need[i] and not (Kd is None and n in ("K_bar", "Xbar_bar"))
                         and not (n == "w_bar" and not ctx.has_w))
            if not want:
                return (None,) * 9
            seeds = [None if t is None else t.detach().to(torch.float64).contiguous() for t in (Jb, Xb, Ub)]
            o = s.policy_rollout_adjoint_device(pd, ud, Xd, Kd, ctx.X, *seeds, lbx=lo, ubx=hi, want=want)
            B = ctx.X.shape[0]

            def grad(i, n, like):  # a shared input's gradient is the sum over the scenarios
                g = o.get(n)
                if g is None:
                    return None
                if n == "K_bar" and ctx.k_view:
                    g = g.transpose(-1, -2)
                return g.sum(0) if like.dim() == g.dim() - 1 and g.shape[0] == B else g

            return (None, grad(1, "p_bar", pd), grad(2, "ubar_bar", ud), grad(3, "Xbar_bar", Xd),
                    None if Kd is None else grad(4, "K_bar", Kd), o.get("e0_bar"), o.get("w_bar"), None, None)

    return _Rollout


def policy_rollout(solver, p, ubar, Xbar, K, e0, w=None, lbx=None, ubx=None):
    """M disturbance rollouts per scenario of the clamped policy (:meth:`Solver.policy_rollout_device`,
    whose shapes the arguments have; CUDA float64 tensors, ``e0`` (B,M,nx) and ``w`` (B,M,N,nx) with
    the B) as a differentiable function: returns ``J`` (B,M), ``X`` (B,M,N+1,nx) and the applied
    controls ``U`` (B,M,N,nu), through which ``backward`` reaches ``p``, ``ubar``, ``Xbar``, ``K``,
    ``e0`` and ``w`` -- each only if it requires grad -- by one
    :meth:`Solver.policy_rollout_adjoint_device` launch.  The clamp bounds ``lbx`` / ``ubx`` get no
    gradient, and ``viol``, a maximum, is not an output.  A control the clamp changed passes no
    gradient (u_raw exactly on a bound counts as unclamped).  Neither pass copies to the host or
    synchronises."""
    return _rollout_function().apply(solver, p, ubar, Xbar, K, e0, w, lbx, ubx)


@functools.lru_cache(maxsize=None)
def _covariance_function():
    import torch

    from . import policy

    def fold(G):  # the forward reads the entries i >= j of a column-major block: [..., j, i] with i >= j
        return torch.triu(G + G.transpose(-1, -2), 1) + torch.diag_embed(torch.diagonal(G, dim1=-2, dim2=-1))

    class _Covariance(torch.autograd.Function):
        @staticmethod
        def forward(ctx, solver, p, ubar, Xbar, K, S0, W, obs_var):
            det = [None if t is None else t.detach().contiguous() for t in (p, ubar, Xbar, K, S0, W, obs_var)]
            pd, ud, Xd, Kd, Sd, Wd, od = det
            _, nu, nx = solver._policy_dims()
            ctx.k_view = Kd is not None and tuple(Kd.shape[-2:]) == (nu, nx)
            if ctx.k_view:  # policy_device's view (…, nu, nx): to the kernel's column-major blocks
                Kd = Kd.transpose(-1, -2).contiguous()
            r = solver.policy_covariance_device(pd, ud, Xd, Kd, Sd, W=Wd, obs_var=od, want=("Sigma", "sigma_u", "sigma_g"))
            ctx.set_materialize_grads(False)  # an output the loss does not read seeds nothing
            ctx.solver, ctx.ins, ctx.res = solver, (pd, ud, Xd, Kd, Sd, Wd, od), r
            return r["Sigma"], r["sigma_u"], r["sigma_g"]

        @staticmethod
        def backward(ctx, Sb, sub, sgb):
            s = ctx.solver
            pd, ud, Xd, Kd, Sd, Wd, od = ctx.ins
            if Kd is None:
                sub = None  # sigma_u is identically 0 in the open loop
            if Sb is None and sub is None and sgb is None:
                return (None,) * 8
            need = ctx.needs_input_grad  # (solver, p, ubar, Xbar, K, S0, W, obs_var)
            names = ((1, "p_bar"), (2, "ubar_bar"), (3, "Xbar_bar"), (4, "K_bar"), (5, "S0_bar"), (6, "W_bar"),
                     (7, "obs_var_bar"))
            want = tuple(n for i, n in names if need[i] and ctx.ins[i - 1] is not None)
            if not want:
                return (None,) * 8
            r = ctx.res
            f64 = lambda t: None if t is None else t.detach().to(torch.float64).contiguous()  # noqa: E731
            vu = None if sub is None else policy.var_seed(r["sigma_u"], f64(sub)).contiguous()
            vg = None if sgb is None else policy.var_seed(r["sigma_g"], f64(sgb)).contiguous()
            o = s.policy_covariance_adjoint_device(pd, ud, Xd, Kd, r["Sigma"], Sigma_bar=f64(Sb), var_u_bar=vu,
                                                   var_g_bar=vg, want=want)
            B = r["Sigma"].shape[0]

            def grad(n, like, per_case=False):
                """Output n summed over the cases (unless the input has them) and, for an input the
                batch shares, over the scenarios."""
                g = o.get(n)
                if g is None:
                    return None
                if n == "K_bar" and ctx.k_view:
                    g = g.transpose(-1, -2)
                if n in ("S0_bar", "W_bar"):
                    g = fold(g)
                if not per_case:
                    g = g.sum(1)
                return g.sum(0) if like.dim() == g.dim() - 1 else g

            return (None, grad("p_bar", pd), grad("ubar_bar", ud), grad("Xbar_bar", Xd),
                    None if Kd is None else grad("K_bar", Kd), grad("S0_bar", Sd, True),
                    None if Wd is None else grad("W_bar", Wd, True), None if od is None else grad("obs_var_bar", od))

    return _Covariance


def policy_covariance(solver, p, ubar, Xbar, K, S0, W=None, obs_var=None):
    """The closed-loop covariance of the policy (:meth:`Solver.policy_covariance_device`, whose shapes
    the arguments have; CUDA float64 tensors) as a differentiable function: returns ``Sigma``
    (B,nc,N+1,nx,nx), ``sigma_u`` (B,nc,N,nu) and ``sigma_g`` (B,nc,N+1,m), through which ``backward``
    reaches ``p``, ``ubar``, ``Xbar``, ``K``, ``S0``, ``W`` and ``obs_var`` -- each only if it requires
    grad -- by one :meth:`Solver.policy_covariance_adjoint_device` launch; the square roots' chain rule
    is :func:`nmpc_amd.policy.var_seed` (a deviation that is exactly 0 passes no gradient).  The
    forward reads only the entries i >= j of ``S0`` and ``W``, so their gradients are folded onto those
    entries: an off-diagonal one gets G_ij + G_ji, the diagonal G_ii and the unread triangle 0 --
    perturbing one stored entry gives what autograd reports.  An input shared by the cases or by the
    batch gets the sum.  Neither pass copies to the host or synchronises."""
    return _covariance_function().apply(solver, p, ubar, Xbar, K, S0, W, obs_var)


def solve(solver, p, lbx, ubx, lbg, ubg, x0=None, backward="host"):
    """Solves the batch at the parameters ``p`` -- a (B, np) float64 CUDA tensor that may require
    grad -- and returns the solution ``x`` (B, nw) and its state trajectory ``X`` (B, nx(N+1)) as
    CUDA tensors through which ``backward`` reaches p.  ``lbx``, ``ubx``, ``lbg``, ``ubg`` are
    host arrays as :meth:`Solver.__call__` takes them ((n,) or (n,B)); ``x0`` is a (B, nw) CUDA
    tensor, absent = zeros.  A scenario that did not converge (status not 0 or 1), or whose KKT
    matrix does not factorise along the delta ladder (``info`` 1), gets a NaN row in p's gradient.
    Equality rows raise in backward, as :meth:`Solver.barrier_weights` does.

    ``backward="device"`` keeps the solution, the bounds and the status on the device and runs
    backward as one :meth:`Solver.sensitivity_adjoint_device` launch: neither pass copies to the
    host or synchronises, so the layer can be enqueued behind other work.  The NaN rows are then
    applied on the device, and an equality row gives a NaN row (``info`` -11) instead of raising.
    The default ``"host"`` is the three-launch route of :meth:`Solver.sensitivity_adjoint`.

    With a ``torch.autograd.forward_ad`` dual tensor for ``p`` the returned x and X carry the
    tangents dx* and dX* for p's tangent (one direction per scenario): with ``backward="device"``
    one :meth:`Solver.sensitivity_device` launch and a ``torch.where`` for the NaN rows, otherwise
    :meth:`Solver.sensitivity_fused`."""
    if backward not in ("host", "device"):
        raise ValueError(f"backward: expected 'host' or 'device', got {backward!r}")
    return _function().apply(p, solver, lbx, ubx, lbg, ubg, x0, backward == "device")
