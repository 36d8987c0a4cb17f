"""Applying the plan's feedback policy between two solves.

:meth:`nmpc_amd.nlpsol.Solver.policy_device` returns, per scenario, the stage gains K_k, the
feedforward kff_k per parameter direction and the plan's states X*_k; :func:`apply` evaluates

    u_k(x, c) = u*_k + K_k (x - X*_k) + sum_d kff_k^(d) c_d

with torch ops on the caller's stream: nothing is copied to the host."""
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
