"""``nlpsol``-compatible front end over the C-ABI.

Mirrors the reference's operator interface for the hot path:

    solver = ca.nlpsol('solver', 'ipopt', nlp_prob, opts)       Python/NMPC_TT.py:267
    sol = solver(x0=..., lbx=..., ubx=..., lbg=..., ubg=..., p=...)   :358-365
    u = ca.reshape(sol['x'], n_controls, N)                     :367

``nlpsol(name, 'ipopt', spec, opts)`` takes a :class:`ProblemSpec` instead of a
symbolic dict (there is no CasADi here) and the same ``opts`` dict
(``{'ipopt': {...}, 'print_time': 0}``).  The returned :class:`Solver` is
called with the same keyword arguments.  Each argument may be one column
((n,), (n,1)) or a batch of columns ((n,B), CasADi's ``Function.map``
horzcat convention); bounds given as one column are shared by the batch.
Results come back as numpy arrays shaped (n,1) for one scenario or (n,B),
so ``np.reshape(sol['x'], (6, N), order='F')`` is ``ca.reshape``.

Errors follow CasADi: a dimension mismatch raises; non-convergence does not
(it is reported by ``solver.stats()``, which the reference never reads --
SURVEY F8).  All arithmetic runs in the HIP library; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Any

import numpy as np

from . import _lib
from .spec import ProblemSpec

RETURN_STATUS = {
    0: "Solve_Succeeded", 1: "Solved_To_Acceptable_Level", 2: "Infeasible_Problem_Detected",
    3: "Search_Direction_Becomes_Too_Small", 4: "Diverging_Iterates",
    -1: "Maximum_Iterations_Exceeded", -2: "Restoration_Failed", -3: "Error_In_Step_Computation",
    -11: "Invalid_Problem_Definition", -13: "Invalid_Number_Detected",
    -102: "Insufficient_Memory",  # NMPC_STATUS_EQ_UNRESERVED: equality rows, no reserve_equality(B)
}
_SUCCESS = (0, 1)
NOT_RUN = -1000  # NMPC_STATUS_NOT_RUN: a closed-loop step the scheduler never ran
_DP = C.POINTER(C.c_double)
_IP = C.POINTER(C.c_int32)


def _dptr(a: np.ndarray):
    return a.ctypes.data_as(_DP)


def _flat_ins(ins):
    """``[(array, ld)]`` (an absent one ``(None, 0)``) as the flat ``[pointer, ld, ...]``."""
    flat = []
    for a, ld in ins:
        flat += [_dptr(a) if a is not None else None, ld]
    return flat


def _dev_in(t, tail, B, name):
    """``[pointer, ld]`` of a device input: a float64 CUDA tensor of shape (B, *tail), or one the
    batch shares, of shape tail (ld = 0); None gives the null pointer."""
    import torch  # plumbing only: device memory and streams

    if t is None:
        return [C.c_void_p(0), 0]
    assert t.dtype == torch.float64 and t.is_cuda and t.is_contiguous(), name
    if tuple(t.shape) == tuple(tail):
        return [C.c_void_p(t.data_ptr()), 0]
    assert tuple(t.shape) == (B, *tail), (name, tuple(t.shape), (B, *tail))
    return [C.c_void_p(t.data_ptr()), int(np.prod(tail))]


def _dev_ins(fields, B):
    """:func:`_dev_in` of each ``(name, tensor, tail)``, flat."""
    return [v for name, t, tail in fields for v in _dev_in(t, tail, B, name)]


def _dev_outs(out, shapes):
    """Pointers of the given device outputs (null where absent), each checked against its
    shape; info and nsat are int32, every other float64."""
    import torch  # plumbing only

    ptrs = []
    for k, shp in shapes:
        t = out.get(k)
        if t is not None:
            dt = torch.int32 if k in ("info", "nsat") else torch.float64
            assert t.dtype == dt and t.is_cuda and t.is_contiguous() and tuple(t.shape) == tuple(shp), k
        ptrs.append(C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0))
    return ptrs


def _first_out(out, keys, caller):
    """The first of the outputs ``keys`` that ``out`` holds: it carries the batch size."""
    for k in keys:
        if out.get(k) is not None:
            return out[k]
    raise ValueError(f"{caller}: out holds none of " + ", ".join(keys))


def _stream_ptr(stream):
    import torch  # plumbing only

    return C.c_void_p((torch.cuda.current_stream() if stream is None else stream).cuda_stream)


def make_options(opts: dict | None) -> _lib.Options:
    """IPOPT option dict (CasADi ``opts['ipopt']``) -> C options struct."""
    o = _lib.default_options()
    if not opts:
        return o
    ip = dict(opts.get("ipopt", {}))
    if "linear_solver_fp32" in ip or "reserved0" in ip:
        raise ValueError("use the nlpsol option linear_solver_precision='single' (not an IPOPT option)")
    for k, v in ip.items():
        name = _lib.IPOPT_ALIASES.get(k, k)
        if name == "warm_start_init_point":
            if v != "no":
                raise ValueError("only warm_start_init_point='no' (IPOPT default: lam_x0/lam_g0 unused) "
                                 "is supported")
            continue
        if name in ("print_level", "print_timing_statistics", "sb", "linear_solver", "hessian_approximation",
                    "mu_strategy", "nlp_scaling_method", "fixed_variable_treatment"):
            if name == "hessian_approximation" and v != "exact":
                raise ValueError("only hessian_approximation='exact' is supported")
            if name == "mu_strategy" and v != "monotone":
                raise ValueError("only mu_strategy='monotone' (IPOPT default) is supported")
            if name == "nlp_scaling_method" and v != "gradient-based":
                raise ValueError("only nlp_scaling_method='gradient-based' (IPOPT default) is supported")
            if name == "fixed_variable_treatment" and v != "make_parameter":
                raise ValueError("only fixed_variable_treatment='make_parameter' (IPOPT default) is supported")
            continue  # output / linear-solver choices do not change the iterates here
        if not hasattr(o, name):
            raise ValueError(f"unsupported IPOPT option {k!r}")
        setattr(o, name, type(getattr(o, name))(v))
    for k in opts:
        if k not in ("ipopt", "print_time", "verbose", "expand", "error_on_fail", "linear_solver_precision"):
            raise ValueError(f"unsupported nlpsol option {k!r}")
    prec = opts.get("linear_solver_precision", "double")
    if prec not in ("double", "single"):
        raise ValueError("linear_solver_precision must be 'double' or 'single'")
    o.linear_solver_fp32 = 1 if prec == "single" else 0
    return o


class Solver:
    """Callable returned by :func:`nlpsol`; one handle (and GPU) per instance."""

    def __init__(self, name: str, spec: ProblemSpec, opts: dict | None = None):
        spec.validate()
        self.name = name
        self.spec = spec
        self.error_on_fail = bool((opts or {}).get("error_on_fail", False))
        L = _lib.lib()
        d = _lib.Desc()
        d.model = 1 if spec.model == "uav5" else 0
        d.N, d.np, d.n_obs = spec.N, spec.np, spec.n_obs
        d.T, d.w1, d.w2, d.vfov, d.hfov = spec.T, spec.w1, spec.w2, spec.vfov, spec.hfov
        for j, ob in enumerate(spec.obstacles):
            d.obs_x[j], d.obs_y[j], d.obs_rsum[j] = ob.x, ob.y, ob.r
            d.obs_x_pidx[j], d.obs_y_pidx[j] = ob.x_pidx, ob.y_pidx
        d.opts = make_options(opts)
        d.w1_pidx, d.w2_pidx = spec.w1_pidx, spec.w2_pidx
        self.max_iter = int(d.opts.max_iter)
        # IPOPT's unscaled acceptance thresholds, applied by certify()
        self._cert_tol = (float(d.opts.dual_inf_tol), float(d.opts.constr_viol_tol), float(d.opts.compl_inf_tol))
        self._bound_relax = float(d.opts.bound_relax_factor)  # barrier_weights()
        # IPOPT's inertia-correction ladder, applied by sensitivity()
        self._perturb = (float(d.opts.first_hessian_perturbation), float(d.opts.perturb_inc_fact_first),
                         float(d.opts.perturb_inc_fact), float(d.opts.max_hessian_perturbation))
        h = C.c_void_p()
        _lib.check(L.nmpc_create(C.byref(d), C.byref(h)))
        self._h = h
        self._stats: dict[str, Any] = {}
        self.nw, self.ng, self.np, self.nX = spec.nw, spec.ng, spec.np, spec.nX

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                _lib.lib().nmpc_destroy(h)
            except Exception:
                pass
            self._h = None

    # ---- argument normalisation (CasADi DM column / matrix semantics)
    def _arg(self, v, n: int, default: float, name: str):
        if v is None:
            return np.full((1, n), default), 0
        a = np.asarray(v, dtype=np.float64)
        if a.ndim == 0:
            a = np.full((n,), float(a))
        if a.ndim == 1:
            if a.shape[0] != n:
                raise ValueError(f"{name}: expected length {n}, got {a.shape[0]}")
            return np.ascontiguousarray(a.reshape(1, n)), 0
        if a.ndim == 2:
            if a.shape[0] != n:
                raise ValueError(f"{name}: expected {n} rows, got shape {a.shape}")
            cols = np.ascontiguousarray(a.T)  # (B, n): each scenario contiguous
            if cols.shape[0] == 1:
                return cols, 0
            return cols, n
        raise ValueError(f"{name}: expected a vector or an (n,B) matrix")

    @staticmethod
    def _batch(B, name, rows, grow=True):
        """The batch size after an argument of ``rows`` scenarios: it must match B, which (with
        ``grow``) may still be the 1 of shared arguments alone."""
        if rows != B and not (grow and B == 1):
            raise ValueError(f"{name}: batch size {rows} does not match {B}")
        return rows

    def _host_ins(self, fields, B=1, grow=True):
        """NumPy inputs ``[(name, value, n, required)]`` as ``[(array, ld)]`` (an absent optional
        one ``(None, 0)``), and the batch size they carry."""
        ins = []
        for name, v, n, required in fields:
            if v is None:
                if required:
                    raise ValueError(f"{name} is required")
                ins.append((None, 0))
                continue
            a, ld = self._arg(v, n, 0.0, name)
            if ld:
                B = self._batch(B, name, a.shape[0], grow)
            ins.append((a, ld))
        return ins, B

    def _host_seeds(self, fields, B, what, grow=True):
        """Seeds or right-hand sides ``[(name, value, n)]``, each (n,), (n,k) or (n,k,B) or absent,
        as ``[(array, ld)]`` in :meth:`_rhs`' layout, their common k (None: all absent) and B."""
        k, ins = None, []
        for name, r, n in fields:
            if r is None:
                ins.append((None, 0))
                continue
            a, ld, kk = self._rhs(r, n, name)
            if k not in (None, kk):
                raise ValueError(f"{name}: {kk} {what} do not match {k}")
            k = kk
            if ld:
                B = self._batch(B, name, a.shape[0], grow)
            ins.append((a, ld))
        return ins, k, B

    def __call__(self, x0=None, lbx=None, ubx=None, lbg=None, ubg=None, p=None, lam_x0=None, lam_g0=None):
        # lam_x0 / lam_g0 are accepted and, exactly as IPOPT does under its default
        # warm_start_init_point='no' (the reference sets no warm-start option,
        # Python/NMPC_TT.py:257-265), not used: the multipliers are initialised by
        # IPOPT's own rules (bound_mult_init_val, least-squares y).  Their shapes are
        # still checked as CasADi checks them.
        for name, v, n in (("lam_x0", lam_x0, self.nw), ("lam_g0", lam_g0, self.ng)):
            if v is not None:
                self._arg(v, n, 0.0, name)
        args = {}
        B = 1
        for name, v, n, dflt in (("x0", x0, self.nw, 0.0), ("lbx", lbx, self.nw, -np.inf),
                                 ("ubx", ubx, self.nw, np.inf), ("lbg", lbg, self.ng, -np.inf),
                                 ("ubg", ubg, self.ng, np.inf), ("p", p, self.np, 0.0)):
            a, ld = self._arg(v, n, dflt, name)
            if ld:
                if B not in (1, a.shape[0]):
                    raise ValueError(f"{name}: batch size {a.shape[0]} does not match {B}")
                B = a.shape[0]
            args[name] = (a, ld)
        out = self.solve_batch(B, **{k: v for k, v in args.items()})
        single = B == 1
        res = {}
        for k in ("x", "g", "lam_x", "lam_g", "lam_p", "X"):
            arr = out[k].T  # (n, B)
            res[k] = arr if not single else arr.reshape(-1, 1)
        res["f"] = out["f"].reshape(1, B) if not single else out["f"].reshape(1, 1)
        st = out["status"]
        self._stats = {
            "return_status": RETURN_STATUS.get(int(st[0]), str(int(st[0]))) if single
            else [RETURN_STATUS.get(int(s), str(int(s))) for s in st],
            "success": bool(st[0] in _SUCCESS) if single else [bool(s in _SUCCESS) for s in st],
            "iter_count": int(out["iters"][0]) if single else out["iters"].copy(),
            "status_code": st.copy(),
        }
        if self.error_on_fail and not np.all(np.isin(st, _SUCCESS)):
            raise RuntimeError(f"nlpsol '{self.name}' failed: {self._stats['return_status']}")
        return res

    def solve_batch(self, B: int, x0, lbx, ubx, lbg, ubg, p):
        """Arrays as (B or 1, n) C-contiguous + leading dim (0 = broadcast)."""
        L = _lib.lib()
        out = {
            "x": np.empty((B, self.nw)), "g": np.empty((B, self.ng)), "lam_x": np.empty((B, self.nw)),
            "lam_g": np.empty((B, self.ng)), "lam_p": np.empty((B, self.np)), "X": np.empty((B, self.nX)),
            "f": np.empty(B),
            "status": np.empty(B, dtype=np.int32), "iters": np.empty(B, dtype=np.int32),
        }
        ins = []
        for a, ld in (x0, lbx, ubx, lbg, ubg, p):
            ins += [_dptr(a), ld]
        _lib.check(L.nmpc_solve_batch(
            self._h, B, *ins, _dptr(out["x"]), _dptr(out["f"]), _dptr(out["g"]), _dptr(out["lam_x"]),
            _dptr(out["lam_g"]), _dptr(out["lam_p"]), _dptr(out["X"]), out["status"].ctypes.data_as(_IP),
            out["iters"].ctypes.data_as(_IP)))
        return out

    def solve_device(self, x0, lbx, ubx, lbg, ubg, p, out: dict, stream=None):
        """Device path: torch CUDA float64 tensors, scenario-major (B, n) or shared (n,).

        ``out`` holds preallocated device tensors x (B,nw) [required], f (B,),
        g (B,ng), lam_x (B,nw), lam_g (B,ng), lam_p (B,np), X (B,nX), status/iters (B,) int32
        (optional).  Enqueued on ``stream`` (torch stream; default = current); never
        synchronises the host.  Batches with equality rows (lbg == ubg) need
        ``reserve_equality(B)`` first, otherwise every scenario reports status -102
        (Insufficient_Memory) with NaN x and f.
        """
        B = out["x"].shape[0]
        ins = _dev_ins((("x0", x0, (self.nw,)), ("lbx", lbx, (self.nw,)), ("ubx", ubx, (self.nw,)),
                        ("lbg", lbg, (self.ng,)), ("ubg", ubg, (self.ng,)), ("p", p, (self.np,))), B)

        def op(k):
            t = out.get(k)
            return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)

        _lib.check(_lib.lib().nmpc_solve_batch_dev(self._h, B, *ins, op("x"), op("f"), op("g"), op("lam_x"),
                                                   op("lam_g"), op("lam_p"), op("X"), op("status"), op("iters"),
                                                   _stream_ptr(stream)))

    # ---- evaluation at given points (nmpc_eval_batch: CasADi's nlp_f / nlp_g / nlp_grad_f)
    def evaluate(self, x, p, lam_g=None, lam_x=None, lbx=None, ubx=None, lbg=None, ubg=None):
        """f, g, X, grad_f and grad_l = grad_f + J_g' lam_g + lam_x at the given decision
        vectors, on the GPU (the reference's ``ff(u, p)``, Python/NMPC_TT.py:368, and the
        ``nlp_f`` / ``nlp_g`` / ``nlp_grad_f`` of a CasADi nlpsol object).  Arguments as
        ``__call__``'s: one column or (n,B); one column is shared by the batch.  Multipliers
        in CasADi's sign convention, absent = zeros.  With any bound given (absent ones are
        infinite) the result also has ``kkt`` (5,B): rows stat = |grad_l|_inf, gmax =
        |grad_f|_inf, viol, compl, lmax (unnormalised; see nmpc_eval_batch_dev)."""
        want_kkt = any(v is not None for v in (lbx, ubx, lbg, ubg))
        if want_kkt:  # an absent bound is infinite
            lbx, lbg = (-np.inf if v is None else v for v in (lbx, lbg))
            ubx, ubg = (np.inf if v is None else v for v in (ubx, ubg))
        ins, B = self._host_ins((("x", x, self.nw, True), ("p", p, self.np, True), ("lam_g", lam_g, self.ng, False),
                                 ("lam_x", lam_x, self.nw, False), ("lbx", lbx, self.nw, False),
                                 ("ubx", ubx, self.nw, False), ("lbg", lbg, self.ng, False),
                                 ("ubg", ubg, self.ng, False)))
        out = {"f": np.empty(B), "g": np.empty((B, self.ng)), "X": np.empty((B, self.nX)),
               "grad_f": np.empty((B, self.nw)), "grad_l": np.empty((B, self.nw))}
        if want_kkt:
            out["kkt"] = np.empty((B, 5))
        _lib.check(_lib.lib().nmpc_eval_batch(
            self._h, B, *_flat_ins(ins), _dptr(out["f"]), _dptr(out["g"]), _dptr(out["X"]), _dptr(out["grad_f"]),
            _dptr(out["grad_l"]), _dptr(out["kkt"]) if want_kkt else None))
        res = {k: v.T for k, v in out.items() if k != "f"}
        res["f"] = out["f"].reshape(1, B)
        return res

    def evaluate_device(self, x, p, out: dict, lam_g=None, lam_x=None, lbx=None, ubx=None, lbg=None, ubg=None,
                        stream=None):
        """Device path of :meth:`evaluate`: torch CUDA float64 tensors, scenario-major (B, n)
        or shared (n,).  ``out`` holds preallocated device tensors, any of f (B,), g (B,ng),
        X (B,nX), grad_f (B,nw), grad_l (B,nw), kkt (B,5) (kkt needs all four bounds).
        Enqueued on ``stream`` (default = current); never synchronises the host."""
        keys = ("f", "g", "X", "grad_f", "grad_l", "kkt")
        B = _first_out(out, keys, "evaluate_device").shape[0]
        ins = _dev_ins((("x", x, (self.nw,)), ("p", p, (self.np,)), ("lam_g", lam_g, (self.ng,)),
                        ("lam_x", lam_x, (self.nw,)), ("lbx", lbx, (self.nw,)), ("ubx", ubx, (self.nw,)),
                        ("lbg", lbg, (self.ng,)), ("ubg", ubg, (self.ng,))), B)
        outs = _dev_outs(out, zip(keys, ((B,), (B, self.ng), (B, self.nX), (B, self.nw), (B, self.nw), (B, 5))))
        _lib.check(_lib.lib().nmpc_eval_batch_dev(self._h, B, *ins, *outs, _stream_ptr(stream)))

    def certify(self, sol: dict, lbx, ubx, lbg, ubg, p):
        """First-order certificate of a result of ``__call__`` that does not come from the
        solver: ``sol['x']``, ``sol['lam_g']``, ``sol['lam_x']`` are re-evaluated on the GPU
        (:meth:`evaluate`) and judged by IPOPT's unscaled acceptance thresholds of this
        solver's options, read on g(x): per scenario
        ``stat`` = |grad f + J' lam_g + lam_x|_inf, ``stat_rel`` = stat / (1 + |grad f|_inf),
        ``viol`` = the largest bound violation, ``compl`` = max |lam| * gap / (1 + |lam|_inf), and
        ``ok`` = stat <= dual_inf_tol and stat_rel <= 1e-4 and viol <= constr_viol_tol and
        compl <= compl_inf_tol.  ``kkt`` is the raw (5,B) array.  A NaN anywhere gives ok = False."""
        ev = self.evaluate(sol["x"], p, lam_g=sol["lam_g"], lam_x=sol["lam_x"], lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg)
        stat, gmax, viol, cpl, lmax = ev["kkt"]
        dual_tol, viol_tol, compl_tol = self._cert_tol
        with np.errstate(invalid="ignore"):
            ok = ((stat <= dual_tol) & (stat <= 1e-4 * (1 + gmax)) & (viol <= viol_tol)
                  & (cpl <= compl_tol * (1 + lmax)))
        return {"stat": stat, "stat_rel": stat / (1 + gmax), "viol": viol, "compl": cpl / (1 + lmax), "ok": ok,
                "kkt": ev["kkt"]}

    # ---- products at given points (nmpc_products_batch: CasADi's nlp_jac_g / nlp_hess_l on vectors)
    def _xpl(self, x, p, lam_g):
        """The inputs every entry point at given points starts with: :meth:`_host_ins`' fields."""
        return ("x", x, self.nw, True), ("p", p, self.np, True), ("lam_g", lam_g, self.ng, False)

    def _xpl_device(self, x, p, lam_g, B):
        return _dev_ins((("x", x, (self.nw,)), ("p", p, (self.np,)), ("lam_g", lam_g, (self.ng,))), B)

    def _products(self, x, p, d, lam_g, obj_factor, want=("jv", "hv", "dX")):
        """d: the directions as :meth:`_dp_dirs` returns them.  Returns (B, nv, n) arrays."""
        ins, B = self._host_ins(self._xpl(x, p, lam_g))
        v, B = self._dp_arg(d, B, "v", grow=True)
        sizes = {"jv": self.ng, "hv": self.nw, "dX": self.nX}
        out = {k: np.empty((B, d.shape[1], sizes[k])) for k in want}
        _lib.check(_lib.lib().nmpc_products_batch(
            self._h, B, d.shape[1], *_flat_ins(ins), float(obj_factor), *_flat_ins([v]),
            *[_dptr(out[k]) if k in out else None for k in ("jv", "hv", "dX")]))
        return out

    def products(self, x, p, v, lam_g=None, obj_factor=1.0):
        """Jacobian- and Hessian-vector products at the given decision vectors, on the GPU:
        ``jv`` (ng,nv,B) = J_g v, ``hv`` (nw,nv,B) = (obj_factor grad^2 f + sum lam_g_i grad^2 g_i) v
        (CasADi's ``hess_l`` convention, lam_g absent = zeros) and ``dX`` (nX,nv,B) = (dX/dw) v,
        the tangent of the rollout.  x, p, lam_g as :meth:`evaluate`'s; ``v`` is one direction
        (nw,), directions (nw,nv) shared by the batch, or (nw,nv,B)."""
        out = self._products(x, p, self._dp_dirs(v, 1, self.nw, "v")[0], lam_g, obj_factor)
        return {k: np.ascontiguousarray(t.transpose(2, 1, 0)) for k, t in out.items()}

    def products_device(self, x, p, v, out: dict, lam_g=None, obj_factor=1.0, stream=None):
        """Device path of :meth:`products`: torch CUDA float64 tensors, x, p, lam_g
        scenario-major (B, n) or shared (n,); ``v`` is (B, nv, nw) or shared (nv, nw); ``out``
        holds preallocated device tensors, any of jv (B,nv,ng), hv (B,nv,nw), dX (B,nv,nX).
        Enqueued on ``stream`` (default = current); never synchronises the host."""
        keys = ("jv", "hv", "dX")
        B, nv = _first_out(out, keys, "products_device").shape[:2]
        outs = _dev_outs(out, zip(keys, ((B, nv, self.ng), (B, nv, self.nw), (B, nv, self.nX))))
        _lib.check(_lib.lib().nmpc_products_batch_dev(
            self._h, B, nv, *self._xpl_device(x, p, lam_g, B), float(obj_factor),
            *_dev_in(v, (nv, self.nw), B, "v"), *outs, _stream_ptr(stream)))

    def jacobian(self, x, p):
        """Dense J_g (ng,nw,B) at the given decision vectors (CasADi's ``nlp_jac_g``): the
        identity directions, shared by the batch, through :meth:`products`' kernel."""
        out = self._products(x, p, np.eye(self.nw), None, 1.0, want=("jv",))
        return np.ascontiguousarray(out["jv"].transpose(2, 1, 0))

    def hessian(self, x, p, lam_g=None, obj_factor=1.0):
        """Dense Hessian of the Lagrangian (nw,nw,B), obj_factor grad^2 f + sum lam_g_i grad^2 g_i
        (CasADi's ``nlp_hess_l``, the full symmetric matrix), column d being W e_d."""
        out = self._products(x, p, np.eye(self.nw), lam_g, obj_factor, want=("hv",))
        return np.ascontiguousarray(out["hv"].transpose(2, 1, 0))

    # ---- parameter-direction products at given points (nmpc_param_products_batch)
    def _param_products(self, x, p, d, lam_g, obj_factor, want=("jp", "hp", "dXp", "gp")):
        """d: the directions as :meth:`_dp_dirs` returns them, or None for none (nd = 0).
        Returns (B, nd, n) arrays, and gp as (B, np)."""
        ins, B = self._host_ins(self._xpl(x, p, lam_g))
        dp, B = ((None, 0), B) if d is None else self._dp_arg(d, B, grow=True)
        nd = 0 if d is None else d.shape[1]
        sizes = {"jp": self.ng, "hp": self.nw, "dXp": self.nX}
        out = {k: np.empty((B, nd, sizes[k])) for k in want if k != "gp"}
        if "gp" in want:
            out["gp"] = np.empty((B, self.np))
        _lib.check(_lib.lib().nmpc_param_products_batch(
            self._h, B, nd, *_flat_ins(ins), float(obj_factor), *_flat_ins([dp]),
            *[_dptr(out[k]) if k in out else None for k in ("jp", "hp", "dXp", "gp")]))
        return out

    def param_products(self, x, p, dp, lam_g=None, obj_factor=1.0):
        """Exact products with the parameter derivatives at the given points, on the GPU, with
        L = obj_factor f + lam_g' g: ``jp`` (ng,nd,B) = (dg/dp) dp, ``hp`` (nw,nd,B) =
        (d_p grad_w L) dp (the change of :meth:`evaluate`'s ``grad_l`` with p at fixed x, lam_g),
        ``dXp`` (nX,nd,B) = (dX/dp) dp, and ``gp`` (np,B) = grad_p L (the negative of a solve's
        ``lam_p`` at its x, lam_g).  x, p, lam_g as :meth:`evaluate`'s; ``dp`` is one direction
        (np,), directions (np,nd) shared by the batch, or (np,nd,B).  Entries of p that nothing
        reads give exactly 0 in gp, and their entries of dp are never read.  ``dp=None`` asks
        for ``gp`` alone (no directions)."""
        if dp is None:
            out = self._param_products(x, p, None, lam_g, obj_factor, want=("gp",))
            return {"gp": np.ascontiguousarray(out["gp"].T)}
        out = self._param_products(x, p, self._dp_dirs(dp, 1)[0], lam_g, obj_factor)
        return {k: np.ascontiguousarray(t.transpose(2, 1, 0) if t.ndim == 3 else t.T) for k, t in out.items()}

    def param_products_device(self, x, p, dp, out: dict, lam_g=None, obj_factor=1.0, stream=None):
        """Device path of :meth:`param_products`: torch CUDA float64 tensors, x, p, lam_g
        scenario-major (B, n) or shared (n,); ``dp`` is (B, nd, np) or shared (nd, np), or None
        when only gp is asked for; ``out`` holds preallocated device tensors, any of jp (B,nd,ng),
        hp (B,nd,nw), dXp (B,nd,nX), gp (B,np).  Enqueued on ``stream`` (default = current);
        never synchronises the host."""
        keys = ("jp", "hp", "dXp", "gp")
        first = _first_out(out, keys, "param_products_device")
        if first is not out.get("gp") and dp is None:
            raise ValueError("param_products_device: dp is required for a directional output")
        B, nd = first.shape[0], (0 if dp is None else dp.shape[-2])
        outs = _dev_outs(out, zip(keys, ((B, nd, self.ng), (B, nd, self.nw), (B, nd, self.nX), (B, self.np))))
        _lib.check(_lib.lib().nmpc_param_products_batch_dev(
            self._h, B, nd, *self._xpl_device(x, p, lam_g, B), float(obj_factor),
            *_dev_in(dp, (nd, self.np), B, "dp"), *outs, _stream_ptr(stream)))

    def param_jacobian(self, x, p):
        """Dense dg/dp (ng,np,B) at the given points: the identity directions, shared by the
        batch, through :meth:`param_products`' kernel."""
        out = self._param_products(x, p, np.eye(self.np), None, 1.0, want=("jp",))
        return np.ascontiguousarray(out["jp"].transpose(2, 1, 0))

    def param_cross(self, x, p, lam_g=None, obj_factor=1.0):
        """Dense d_p grad_w L (nw,np,B), L = obj_factor f + lam_g' g, column d being the
        derivative with respect to p_d (its transpose applied to y serves reverse mode)."""
        out = self._param_products(x, p, np.eye(self.np), lam_g, obj_factor, want=("hp",))
        return np.ascontiguousarray(out["hp"].transpose(2, 1, 0))

    # ---- adjoint (transposed) products at given points (nmpc_adjoint_products_batch)
    def adjoint_products(self, x, p, y=None, z=None, Xbar=None, lam_g=None, obj_factor=1.0,
                         want=("wbar", "pbar")):
        """Exact vector-Jacobian products of the map (w, p) -> (g, grad_w L, X) at the given
        points, on the GPU, with L = obj_factor f + lam_g' g and W its Hessian in w:
        ``wbar`` (nw,na,B) = J' y + W z + (dX/dw)' Xbar and ``pbar`` (np,na,B) = (dg/dp)' y +
        (d_p grad_w L)' z + (dX/dp)' Xbar -- the transposes of :meth:`products` and
        :meth:`param_products`, what reverse mode needs, without forming a matrix.  x, p, lam_g
        as :meth:`evaluate`'s; each seed ``y`` (ng rows), ``z`` (nw), ``Xbar`` (nX) is one seed
        (n,), seeds (n,na) shared by the batch, or (n,na,B); an absent seed contributes nothing,
        at least one is required and all given ones carry the same na.  Entries of p that
        nothing reads give exactly 0 in pbar.  ``want`` names the outputs to form."""
        ins, B = self._host_ins(self._xpl(x, p, lam_g))
        seeds, na, B = self._host_seeds((("y", y, self.ng), ("z", z, self.nw), ("Xbar", Xbar, self.nX)), B, "seeds")
        if na is None:
            raise ValueError("y, z or Xbar is required")
        want = tuple(want)
        if not want or any(k not in ("wbar", "pbar") for k in want):
            raise ValueError(f"want: expected 'wbar' and / or 'pbar', got {want!r}")
        sizes = {"wbar": self.nw, "pbar": self.np}
        out = {k: np.empty((B, na, sizes[k])) for k in ("wbar", "pbar") if k in want}
        _lib.check(_lib.lib().nmpc_adjoint_products_batch(
            self._h, B, na, *_flat_ins(ins), float(obj_factor), *_flat_ins(seeds),
            *[_dptr(out[k]) if k in out else None for k in ("wbar", "pbar")]))
        return {k: np.ascontiguousarray(t.transpose(2, 1, 0)) for k, t in out.items()}

    def adjoint_products_device(self, x, p, out: dict, y=None, z=None, Xbar=None, lam_g=None, obj_factor=1.0,
                                stream=None):
        """Device path of :meth:`adjoint_products`: torch CUDA float64 tensors, x, p, lam_g
        scenario-major (B, n) or shared (n,); each seed is (B, na, n) or shared (na, n), or None;
        ``out`` holds preallocated device tensors, wbar (B,na,nw) and / or pbar (B,na,np).
        Enqueued on ``stream`` (default = current); never synchronises the host."""
        keys = ("wbar", "pbar")
        first = _first_out(out, keys, "adjoint_products_device")
        if y is None and z is None and Xbar is None:
            raise ValueError("y, z or Xbar is required")
        B, na = first.shape[:2]
        seeds = _dev_ins((("y", y, (na, self.ng)), ("z", z, (na, self.nw)), ("Xbar", Xbar, (na, self.nX))), B)
        outs = _dev_outs(out, zip(keys, ((B, na, self.nw), (B, na, self.np))))
        _lib.check(_lib.lib().nmpc_adjoint_products_batch_dev(
            self._h, B, na, *self._xpl_device(x, p, lam_g, B), float(obj_factor), *seeds, *outs, _stream_ptr(stream)))

    # ---- condensed KKT solves at given points (nmpc_kkt_solve_batch: the Newton-step operator)
    def _rhs(self, r, n: int, name: str):
        """(n,), (n,nr) or (n,nr,B) -> ((1 or B, nr, n) C-contiguous, leading dimension, nr)."""
        a = np.asarray(r, dtype=np.float64)
        if a.ndim == 1:
            a = a.reshape(-1, 1)
        if a.ndim not in (2, 3) or a.shape[0] != n or a.shape[1] < 1:
            raise ValueError(f"{name}: expected ({n},), ({n},nr) or ({n},nr,B), got shape {a.shape}")
        nr = a.shape[1]
        if a.ndim == 2:
            return np.ascontiguousarray(a.T).reshape(1, nr, n), 0, nr
        return np.ascontiguousarray(a.transpose(2, 1, 0)), n * nr, nr

    def kkt_solve(self, x, p, r_w=None, r_g=None, lam_g=None, obj_factor=1.0, sigma_x=None, sigma_s=None,
                  delta=None):
        """Solves with the condensed KKT matrix at the given decision vectors, on the GPU:
        ``M dw = r_w + J' r_g`` with ``M = W + diag(sigma_x) + delta I + J' diag(sigma_s + delta) J``
        and W the Hessian of :meth:`hessian` (same ``lam_g`` / ``obj_factor``), by the solver's
        Riccati factorisation.  x, p, lam_g as :meth:`evaluate`'s; ``sigma_x`` (nw,) or (nw,B)
        and ``sigma_s`` (ng,) or (ng,B) are non-negative weights (absent = zeros; ``+inf`` in
        sigma_x fixes the variable: its dw is exactly 0); ``delta`` a scalar or (B,).  ``r_w`` /
        ``r_g`` are one right-hand side (n,), several (n,nr) shared by the batch, or (n,nr,B);
        one of them may be absent (zeros).  Returns ``dw`` (nw,nr,B), ``dX`` (nX,nr,B) the state
        step, ``jdw`` (ng,nr,B) = J dw and ``info`` (B,): 0 = factorised with the right inertia
        (M positive definite), 1 = wrong inertia or singular, -11 = invalid weights; with 1 or
        -11 the scenario's other outputs are NaN."""
        if r_w is None and r_g is None:
            raise ValueError("r_w or r_g is required")
        ins, B = self._host_ins(self._xpl(x, p, lam_g) + (("sigma_x", sigma_x, self.nw, False),
                                                          ("sigma_s", sigma_s, self.ng, False)))
        dl = (None, 0)
        if delta is not None:
            d = np.ascontiguousarray(np.asarray(delta, dtype=np.float64).reshape(-1))
            dl = (d, 0 if d.shape[0] == 1 else 1)
            if dl[1]:
                B = self._batch(B, "delta", d.shape[0])
        rhs, nr, B = self._host_seeds((("r_w", r_w, self.nw), ("r_g", r_g, self.ng)), B, "right-hand sides")
        out = {"dw": np.empty((B, nr, self.nw)), "dX": np.empty((B, nr, self.nX)), "jdw": np.empty((B, nr, self.ng))}
        info = np.empty(B, dtype=np.int32)
        _lib.check(_lib.lib().nmpc_kkt_solve_batch(
            self._h, B, nr, *_flat_ins(ins[:3]), float(obj_factor), *_flat_ins(ins[3:] + [dl] + rhs),
            _dptr(out["dw"]), _dptr(out["dX"]), _dptr(out["jdw"]), info.ctypes.data_as(_IP)))
        res = {k: np.ascontiguousarray(t.transpose(2, 1, 0)) for k, t in out.items()}
        res["info"] = info
        return res

    def kkt_solve_device(self, x, p, out: dict, r_w=None, r_g=None, lam_g=None, obj_factor=1.0, sigma_x=None,
                         sigma_s=None, delta=None, stream=None):
        """Device path of :meth:`kkt_solve`: torch CUDA float64 tensors, x, p, lam_g, sigma_x,
        sigma_s scenario-major (B, n) or shared (n,); ``delta`` (B,) or shared (1,); ``r_w`` is
        (B, nr, nw) or shared (nr, nw), ``r_g`` (B, nr, ng) or (nr, ng); ``out`` holds
        preallocated device tensors, any of dw (B,nr,nw), dX (B,nr,nX), jdw (B,nr,ng) and
        info (B,) int32 (at least one of the first three).  Enqueued on ``stream`` (default =
        current); never synchronises the host."""
        keys = ("dw", "dX", "jdw")
        first = _first_out(out, keys, "kkt_solve_device")
        if r_w is None and r_g is None:
            raise ValueError("r_w or r_g is required")
        B, nr = first.shape[:2]
        if delta is not None and tuple(delta.shape) == (1,):
            delta = delta.reshape(())  # shared
        rest = _dev_ins((("sigma_x", sigma_x, (self.nw,)), ("sigma_s", sigma_s, (self.ng,)), ("delta", delta, ()),
                         ("r_w", r_w, (nr, self.nw)), ("r_g", r_g, (nr, self.ng))), B)
        outs = _dev_outs(out, (("dw", (B, nr, self.nw)), ("dX", (B, nr, self.nX)), ("jdw", (B, nr, self.ng)),
                               ("info", (B,))))
        _lib.check(_lib.lib().nmpc_kkt_solve_batch_dev(
            self._h, B, nr, *self._xpl_device(x, p, lam_g, B), float(obj_factor), *rest, *outs, _stream_ptr(stream)))

    def barrier_weights(self, sol: dict, lbx, ubx, lbg, ubg):
        """The barrier weights Sigma_x (nw,B) and Sigma_s (ng,B) at a result of ``__call__``,
        from its signed multipliers (CasADi: negative towards the lower bound):
        ``sigma = max(-lam, 0) / max(v - lo, eps) + max(lam, 0) / max(hi - v, eps)`` with
        ``eps = bound_relax_factor * max(1, |bound|)`` of this solver's options (the amount
        IPOPT moves the bound outwards, so the slack of an active bound is not 0).  A fixed
        variable (lbx == ubx) gets ``+inf``, which :meth:`kkt_solve` takes as "leaves the
        system"; an equality row (lbg == ubg) raises: it needs the augmented system."""
        def weights(v, lam, lo, hi, n, name):
            v, lam = np.asarray(v, dtype=np.float64).reshape(n, -1), np.asarray(lam, dtype=np.float64).reshape(n, -1)
            lo = np.asarray(lo, dtype=np.float64).reshape(n, -1) * np.ones_like(v)
            hi = np.asarray(hi, dtype=np.float64).reshape(n, -1) * np.ones_like(v)
            brf = self._bound_relax
            with np.errstate(invalid="ignore"):
                sl = np.maximum(v - lo, brf * np.maximum(1.0, np.abs(lo)))
                su = np.maximum(hi - v, brf * np.maximum(1.0, np.abs(hi)))
                s = np.maximum(-lam, 0.0) / sl + np.maximum(lam, 0.0) / su
            return s, lo == hi

        sx, fx = weights(sol["x"], sol["lam_x"], lbx, ubx, self.nw, "x")
        ss, eq = weights(sol["g"], sol["lam_g"], lbg, ubg, self.ng, "g")
        if np.any(eq):
            raise ValueError("barrier_weights: equality rows (lbg == ubg) are not supported")
        sx[fx] = np.inf
        return sx, ss

    def sensitivity(self, sol: dict, lbx, ubx, lbg, ubg, p, dp, fd_step: float = 1e-3, tangent: str = "fd"):
        """First-order change of a solution with the parameters: ``dx`` (nw,nd,B) = dx*/dp dp_d
        and ``dlam_g`` (ng,nd,B) for the directions ``dp`` (np,), (np,nd) or (np,nd,B), with
        ``info`` (B,) of :meth:`kkt_solve` and the ``delta`` (B,) used.  With W at
        (x*, lam_g*) and the weights of :meth:`barrier_weights`,

            M dx = -(d_p grad_w L) dp - J' Sigma_s (d_p g) dp,   dlam_g = Sigma_s (J dx + d_p g dp)

        i.e. the interior-point linearisation of the optimality conditions at the returned
        point: rows and bounds with a zero multiplier do not constrain the step, active ones
        hold it with stiffness lam / slack.  M is taken at delta = 0 where it factorises with
        the right inertia.  Where it does not -- M is singular whenever a variable has no
        cost, row or active bound (this model's last heading-rate control moves only the final
        heading, which nothing depends on), and a solution converged to 1e-8 can leave M
        indefinite by as much -- the scenario is solved again as IPOPT's inertia correction
        does: delta = first_hessian_perturbation, then times perturb_inc_fact_first, then
        times perturb_inc_fact, up to max_hessian_perturbation (``info`` stays 1 beyond it).
        A direction M does not determine comes out near 0.  The two parameter derivatives are central
        differences of :meth:`evaluate`'s ``grad_l`` and ``g`` at p +- fd_step * dp_d, at fixed
        (x, lam_g).  Their errors per unit dp: truncation fd_step^2 |d_p^3| / 6, and rounding
        2.2e-16 |terms of grad_l| / fd_step.  At a solution the terms of grad_l cancel (grad f +
        J' lam_g = -lam_x) by two to three orders, so keeping the rounding below 1e-10 of the
        right-hand side needs fd_step >= 2e-4 ... 8e-4 (measured on race_track_2 solutions);
        the default 1e-3 costs a truncation of 1.7e-7 |d_p^3|, at the level of what the
        solve's own 1e-8 tolerance does to the result.  Scale dp so that fd_step * dp is a small move of p.  ``tangent="exact"``
        takes both parameter derivatives from one :meth:`param_products` call instead (``hp`` and
        ``jp`` alone, at (x*, lam_g*)): no difference step, ``fd_step`` is ignored, and the weights,
        the delta ladder and the outputs are the same."""
        if tangent not in ("fd", "exact"):
            raise ValueError(f"tangent: expected 'fd' or 'exact', got {tangent!r}")
        d = np.asarray(dp, dtype=np.float64)
        if d.ndim == 1:
            d = d.reshape(-1, 1)
        if d.ndim not in (2, 3) or d.shape[0] != self.np:
            raise ValueError(f"dp: expected ({self.np},), ({self.np},nd) or ({self.np},nd,B), got shape {d.shape}")
        x = np.asarray(sol["x"], dtype=np.float64).reshape(self.nw, -1)
        lam = np.asarray(sol["lam_g"], dtype=np.float64).reshape(self.ng, -1)
        B, nd = x.shape[1], d.shape[1]
        P = np.asarray(p, dtype=np.float64).reshape(self.np, -1) * np.ones((1, B))
        if d.ndim == 2:
            d = np.repeat(d[:, :, None], B, axis=2)
        sx, ss = self.barrier_weights(sol, lbx, ubx, lbg, ubg)
        if tangent == "exact":
            pp = self._param_products(x, P, d, lam, 1.0, want=("jp", "hp"))
            dgl, dg = (np.ascontiguousarray(pp[k].transpose(2, 1, 0)) for k in ("hp", "jp"))
        else:
            dgl, dg = np.empty((self.nw, nd, B)), np.empty((self.ng, nd, B))
            for j in range(nd):
                ep = self.evaluate(x, P + fd_step * d[:, j, :], lam_g=lam)
                em = self.evaluate(x, P - fd_step * d[:, j, :], lam_g=lam)
                dgl[:, j, :] = (ep["grad_l"] - em["grad_l"]) / (2 * fd_step)
                dg[:, j, :] = (ep["g"] - em["g"]) / (2 * fd_step)
        r, delta = self._kkt_ladder(x, P, -dgl, -(ss[:, None, :] * dg), lam, sx, ss)
        return {"dx": r["dw"], "dlam_g": ss[:, None, :] * (r["jdw"] + dg), "info": r["info"], "delta": delta}

    def _kkt_ladder(self, x, P, r_w, r_g, lam, sx, ss):
        """:meth:`kkt_solve` at delta = 0, and again for the scenarios whose M does not factorise
        with the right inertia along IPOPT's inertia-correction ladder (see :meth:`sensitivity`).
        Returns the last solve's result and the delta (B,) used."""
        first, inc_first, inc, dmax = self._perturb
        delta = np.zeros(x.shape[1])
        while True:
            r = self.kkt_solve(x, P, r_w=r_w, r_g=r_g, lam_g=lam, sigma_x=sx, sigma_s=ss, delta=delta)
            retry = r["info"] == 1
            nxt = np.where(delta == 0.0, first, np.where(delta == first, inc_first * delta, inc * delta))
            retry &= nxt <= dmax
            if not np.any(retry):
                break
            delta = np.where(retry, nxt, delta)
        return r, delta

    def sensitivity_adjoint(self, sol: dict, lbx, ubx, lbg, ubg, p, x_bar=None, lam_g_bar=None, X_bar=None):
        """Reverse mode of :meth:`sensitivity` with ``tangent="exact"``: for seeds ``x_bar`` on
        x*, ``lam_g_bar`` on lam_g* and ``X_bar`` on X* -- each (n,), (n,na) or (n,na,B), absent
        = zeros, at least one given -- ``pbar`` (np,na,B) with <pbar, dp> = <x_bar, dx> +
        <lam_g_bar, dlam_g> + <X_bar, dX*> for every dp, at the cost of one right-hand side per
        seed whatever np is.  The same barrier weights and delta ladder as :meth:`sensitivity`
        (``info`` (B,), ``delta`` (B,)); M is symmetric, so with q = M^-1 (x_bar + (dX/dw)' X_bar
        + J' Sigma_s lam_g_bar)

            pbar = -(d_p grad_w L)' q + (dg/dp)' Sigma_s (lam_g_bar - J q) + (dX/dp)' X_bar

        by :meth:`adjoint_products` at (x*, lam_g*); ``q`` (nw,na,B) and ``jq`` (ng,na,B) = J q
        are returned beside it.  A fixed variable (lbx == ubx) ignores its
        x_bar; a scenario whose ``info`` stays 1 gets NaN; equality rows raise, as
        :meth:`barrier_weights` does."""
        x = np.asarray(sol["x"], dtype=np.float64).reshape(self.nw, -1)
        lam = np.asarray(sol["lam_g"], dtype=np.float64).reshape(self.ng, -1)
        B = x.shape[1]
        P = np.asarray(p, dtype=np.float64).reshape(self.np, -1) * np.ones((1, B))
        seeds, na = {}, None
        for name, v, n in (("x_bar", x_bar, self.nw), ("lam_g_bar", lam_g_bar, self.ng), ("X_bar", X_bar, self.nX)):
            if v is None:
                continue
            a = np.asarray(v, dtype=np.float64)
            if a.ndim == 1:
                a = a.reshape(-1, 1)
            if a.ndim not in (2, 3) or a.shape[0] != n or a.shape[1] < 1 or (a.ndim == 3 and a.shape[2] != B):
                raise ValueError(f"{name}: expected ({n},), ({n},na) or ({n},na,{B}), got shape {a.shape}")
            if na not in (None, a.shape[1]):
                raise ValueError(f"{name}: {a.shape[1]} seeds do not match {na}")
            na = a.shape[1]
            seeds[name] = a if a.ndim == 3 else np.repeat(a[:, :, None], B, axis=2)
        if not seeds:
            raise ValueError("x_bar, lam_g_bar or X_bar is required")
        sx, ss = self.barrier_weights(sol, lbx, ubx, lbg, ubg)
        xb, lb, Xb = seeds.get("x_bar"), seeds.get("lam_g_bar"), seeds.get("X_bar")
        r_w = xb
        if Xb is not None:
            zx = self.adjoint_products(x, P, Xbar=Xb, lam_g=lam, want=("wbar",))["wbar"]
            r_w = zx if xb is None else xb + zx
        sl = None if lb is None else ss[:, None, :] * lb
        r, delta = self._kkt_ladder(x, P, r_w, sl, lam, sx, ss)
        y = -(ss[:, None, :] * r["jdw"]) if sl is None else sl - ss[:, None, :] * r["jdw"]
        pbar = self.adjoint_products(x, P, y=y, z=-r["dw"], Xbar=Xb, lam_g=lam, want=("pbar",))["pbar"]
        pbar[:, :, r["info"] != 0] = np.nan
        return {"pbar": pbar, "info": r["info"], "delta": delta, "q": r["dw"], "jq": r["jdw"]}

    # ---- what the three entry points at a solve's point marshal alike (nmpc_solve_adjoint_batch,
    # nmpc_solve_tangent_batch, nmpc_solve_policy_batch and their _dev twins)
    def _point_fields(self, sol, lbx, ubx, lbg, ubg, p):
        """The nine point inputs in the C argument order: (name, value, length)."""
        return (("x", sol["x"], self.nw), ("p", p, self.np), ("lam_g", sol["lam_g"], self.ng),
                ("lam_x", sol["lam_x"], self.nw), ("g", sol.get("g"), self.ng), ("lbx", lbx, self.nw),
                ("ubx", ubx, self.nw), ("lbg", lbg, self.ng), ("ubg", ubg, self.ng))

    def _point_ins_host(self, sol, lbx, ubx, lbg, ubg, p):
        """NumPy: the nine point inputs as ``[(array, ld)]`` (an absent one ``(None, 0)``), and B
        (x's: every other argument matches it or is shared)."""
        fields = self._point_fields(sol, lbx, ubx, lbg, ubg, p)
        x = self._arg(sol["x"], self.nw, 0.0, "x")
        ins, B = self._host_ins([(*f, False) for f in fields[1:]], x[0].shape[0], grow=False)
        return [x] + ins, B

    def _point_ins_device(self, sol, lbx, ubx, lbg, ubg, p, B=None):
        """torch: the nine point inputs as a flat ``[pointer, ld, ...]``, and B (the outputs'
        when given, else x's)."""
        for k in ("x", "lam_g", "lam_x"):
            if sol.get(k) is None:
                raise ValueError(f"sol: {k} is required")
        if B is None:
            B = sol["x"].shape[0]
        fields = self._point_fields(sol, lbx, ubx, lbg, ubg, p)
        for name, t, n in fields:
            if t is None and name != "g":
                raise ValueError(f"{name} is required")
        return _dev_ins([(name, t, (n,)) for name, t, n in fields], B), B

    def _dp_dirs(self, dp, nd_min, n=None, name="dp"):
        """Directions ``dp`` (np,), (np,nd) or (np,nd,B) -- or ``v``, of length n -- as a float64
        array of 2 or 3 dimensions, and nd."""
        n, cnt = self.np if n is None else n, "n" + name[0]
        d = np.asarray(dp, dtype=np.float64)
        if d.ndim == 1:
            d = d.reshape(-1, 1)
        if d.ndim not in (2, 3) or d.shape[0] != n or d.shape[1] < nd_min:
            raise ValueError(f"{name}: expected ({n},), ({n},{cnt}) or ({n},{cnt},B), got shape {d.shape}")
        return d, d.shape[1]

    def _dp_arg(self, d, B, name="dp", grow=False):
        """:meth:`_dp_dirs`' array in the C layout with its leading dimension, and the batch size."""
        if d.ndim == 3:
            B = self._batch(B, name, d.shape[2], grow)
            return (np.ascontiguousarray(d.transpose(2, 1, 0)), d.shape[0] * d.shape[1]), B  # (B, nd, n)
        return (np.ascontiguousarray(d.T), 0), B  # (nd, n), shared

    def _raise_equality_rows(self, info, lbg, ubg, caller):
        """info = -11 with an equality row: the ``ValueError`` of :meth:`barrier_weights`."""
        if np.any(info == -11):
            lo, hi = (np.asarray(v, dtype=np.float64).reshape(self.ng, -1) for v in (lbg, ubg))
            if np.any(lo == hi):
                raise ValueError(f"{caller}: equality rows (lbg == ubg) are not supported")

    # ---- the same in one launch (nmpc_solve_adjoint_batch: weights, ladder, solves, pullback)
    def sensitivity_adjoint_fused(self, sol: dict, lbx, ubx, lbg, ubg, p, x_bar=None, lam_g_bar=None, X_bar=None):
        """:meth:`sensitivity_adjoint` as one kernel launch: the same arguments, the same dict
        (``pbar`` (np,na,B), ``q`` (nw,na,B), ``jq`` (ng,na,B), ``info`` (B,), ``delta`` (B,)).
        The barrier weights (``sol["g"]`` serves the rows when present, the kernel's own g(x, p)
        otherwise), the delta ladder, the solves and the pullback all run on the device; the
        host only stages the arrays.  Equality rows raise ``ValueError``, as
        :meth:`barrier_weights` does."""
        ins, B = self._point_ins_host(sol, lbx, ubx, lbg, ubg, p)
        seeds, na, _ = self._host_seeds((("x_bar", x_bar, self.nw), ("lam_g_bar", lam_g_bar, self.ng),
                                         ("X_bar", X_bar, self.nX)), B, "seeds", grow=False)
        if na is None:
            raise ValueError("x_bar, lam_g_bar or X_bar is required")
        ins += seeds
        out = {"pbar": np.empty((B, na, self.np)), "q": np.empty((B, na, self.nw)), "jq": np.empty((B, na, self.ng))}
        info, delta = np.empty(B, dtype=np.int32), np.empty(B)
        _lib.check(_lib.lib().nmpc_solve_adjoint_batch(
            self._h, B, na, *_flat_ins(ins), _dptr(out["pbar"]), _dptr(out["q"]), _dptr(out["jq"]),
            info.ctypes.data_as(_IP), _dptr(delta)))
        self._raise_equality_rows(info, lbg, ubg, "sensitivity_adjoint_fused")
        res = {k: np.ascontiguousarray(t.transpose(2, 1, 0)) for k, t in out.items()}
        res["info"], res["delta"] = info, delta
        return res

    def sensitivity_adjoint_device(self, sol: dict, lbx, ubx, lbg, ubg, p, out: dict, x_bar=None, lam_g_bar=None,
                                   X_bar=None, stream=None):
        """Device path of :meth:`sensitivity_adjoint_fused`: torch CUDA float64 tensors.  ``sol``
        holds x (B,nw), lam_g (B,ng), lam_x (B,nw) and optionally g (B,ng) as
        :meth:`solve_device` leaves them; the bounds and ``p`` are scenario-major (B, n) or shared
        (n,); each seed is (B, na, n) or shared (na, n), or None; ``out`` holds preallocated
        device tensors, any of pbar (B,na,np), q (B,na,nw), jq (B,na,ng), info (B,) int32 and
        delta (B,) -- pbar or q at least.  A scenario whose ``info`` is not 0 (1: no rung of the
        delta ladder factorises; -11: an equality row, lbx > ubx or a NaN multiplier) has NaN in
        pbar, q and jq.  Enqueued on ``stream`` (default = current); never synchronises the host
        and reads nothing back."""
        if out.get("pbar") is None and out.get("q") is None:
            raise ValueError("sensitivity_adjoint_device: out holds neither pbar nor q")
        if x_bar is None and lam_g_bar is None and X_bar is None:
            raise ValueError("x_bar, lam_g_bar or X_bar is required")
        B, na = _first_out(out, ("pbar", "q"), "sensitivity_adjoint_device").shape[:2]
        ins, _ = self._point_ins_device(sol, lbx, ubx, lbg, ubg, p, B)
        ins += _dev_ins((("x_bar", x_bar, (na, self.nw)), ("lam_g_bar", lam_g_bar, (na, self.ng)),
                         ("X_bar", X_bar, (na, self.nX))), B)
        outs = _dev_outs(out, (("pbar", (B, na, self.np)), ("q", (B, na, self.nw)), ("jq", (B, na, self.ng)),
                               ("info", (B,)), ("delta", (B,))))
        _lib.check(_lib.lib().nmpc_solve_adjoint_batch_dev(self._h, B, na, *ins, *outs, _stream_ptr(stream)))

    # ---- forward mode in one launch (nmpc_solve_tangent_batch: weights, ladder, parameter
    # products, solves)
    def sensitivity_fused(self, sol: dict, lbx, ubx, lbg, ubg, p, dp):
        """:meth:`sensitivity` with ``tangent="exact"`` as one kernel launch: the same arguments
        (``dp`` (np,), (np,nd) or (np,nd,B)), the same dict (``dx`` (nw,nd,B), ``dlam_g``
        (ng,nd,B), ``info`` (B,), ``delta`` (B,)) and with it ``dX`` (nX,nd,B), the first-order
        change of the state trajectory X*.  The barrier weights (``sol["g"]`` serves the rows
        when present, the kernel's own g(x, p) otherwise), the parameter derivatives, the delta
        ladder and the solves all run on the device; the host only stages the arrays.  A scenario
        whose ``info`` is not 0 has NaN in dx, dlam_g and dX.  Equality rows raise
        ``ValueError``, as :meth:`barrier_weights` does."""
        d, nd = self._dp_dirs(dp, 1)
        ins, B = self._point_ins_host(sol, lbx, ubx, lbg, ubg, p)
        ins.append(self._dp_arg(d, B)[0])
        out = {"dx": np.empty((B, nd, self.nw)), "dlam_g": np.empty((B, nd, self.ng)), "dX": np.empty((B, nd, self.nX))}
        info, delta = np.empty(B, dtype=np.int32), np.empty(B)
        _lib.check(_lib.lib().nmpc_solve_tangent_batch(
            self._h, B, nd, *_flat_ins(ins), _dptr(out["dx"]), _dptr(out["dlam_g"]), _dptr(out["dX"]),
            info.ctypes.data_as(_IP), _dptr(delta)))
        self._raise_equality_rows(info, lbg, ubg, "sensitivity_fused")
        res = {k: np.ascontiguousarray(t.transpose(2, 1, 0)) for k, t in out.items()}
        res["info"], res["delta"] = info, delta
        return res

    def sensitivity_device(self, sol: dict, lbx, ubx, lbg, ubg, p, dp, out: dict, stream=None):
        """Device path of :meth:`sensitivity_fused`: torch CUDA float64 tensors.  ``sol`` holds x
        (B,nw), lam_g (B,ng), lam_x (B,nw) and optionally g (B,ng) as :meth:`solve_device` leaves
        them; the bounds and ``p`` are scenario-major (B, n) or shared (n,); ``dp`` is (B, nd, np)
        or shared (nd, np); ``out`` holds preallocated device tensors, any of dx (B,nd,nw), dlam_g
        (B,nd,ng), dX (B,nd,nX), info (B,) int32 and delta (B,) -- dx, dlam_g or dX at least.  A
        scenario whose ``info`` is not 0 (1: no rung of the delta ladder factorises; -11: an
        equality row, lbx > ubx or a NaN multiplier) has NaN in dx, dlam_g and dX.  Enqueued on
        ``stream`` (default = current); never synchronises the host and reads nothing back."""
        B, nd = _first_out(out, ("dx", "dlam_g", "dX"), "sensitivity_device").shape[:2]
        if dp is None:
            raise ValueError("dp is required")
        ins, _ = self._point_ins_device(sol, lbx, ubx, lbg, ubg, p, B)
        ins += _dev_in(dp, (nd, self.np), B, "dp")
        outs = _dev_outs(out, (("dx", (B, nd, self.nw)), ("dlam_g", (B, nd, self.ng)), ("dX", (B, nd, self.nX)),
                               ("info", (B,)), ("delta", (B,))))
        _lib.check(_lib.lib().nmpc_solve_tangent_batch_dev(self._h, B, nd, *ins, *outs, _stream_ptr(stream)))

    def feedback_gain_device(self, sol: dict, lbx, ubx, lbg, ubg, p, out: dict | None = None, stream=None):
        """Returns ``(K, info)``: the NMPC law's feedback gain K = d u0* / d x0, (B, nu, nx), and
        ``info`` (B,) int32, as CUDA tensors: :meth:`sensitivity_device` for the nx unit directions of p's x0 block,
        shared by every scenario, and the first nu entries of each dx arranged by torch on the
        same stream.  ``sol``, the bounds and ``p`` as :meth:`sensitivity_device` takes them;
        ``out`` may hold a preallocated ``K`` and ``info``.  Between two solves u0* + K (x0' - x0)
        is the law's first-order answer to a measured state x0'.  A scenario whose ``info`` is
        not 0 has NaN in K.  Nothing is copied to the host and nothing synchronises."""
        import torch

        x = sol["x"]
        B, nu, nx = x.shape[0], self.nw // self.spec.N, self.nX // (self.spec.N + 1)
        if stream is None:
            stream = torch.cuda.current_stream()
        with torch.cuda.stream(stream):
            dp = torch.zeros(nx, self.np, dtype=torch.float64, device=x.device)
            dp[:, :nx] = torch.eye(nx, dtype=torch.float64, device=x.device)
            o = {"dx": torch.empty(B, nx, self.nw, dtype=torch.float64, device=x.device),
                 "info": (out or {}).get("info")}
            if o["info"] is None:
                o["info"] = torch.empty(B, dtype=torch.int32, device=x.device)
            self.sensitivity_device(sol, lbx, ubx, lbg, ubg, p, dp, o, stream=stream)
            K = o["dx"][:, :, :nu].transpose(1, 2)  # (B, nu, nx): column j is d u0 / d x0_j
            if (out or {}).get("K") is not None:
                out["K"].copy_(K)
                K = out["K"]
            else:
                K = K.contiguous()
        return K, o["info"]

    def _policy_dims(self):
        N = self.spec.N
        return N, self.nw // N, self.nX // (N + 1)

    def policy_fused(self, sol: dict, lbx, ubx, lbg, ubg, p, dp=None):
        """The feedback policy along the plan through the host entry point
        (``nmpc_solve_policy_batch``): the arguments of :meth:`sensitivity_fused` (``dp`` (np,),
        (np,nd), (np,nd,B) or None for no direction).  Returns NumPy arrays in the C layout's
        order: ``K`` (B,N,nu,nx), ``kff`` (B,nd,N,nu) (None without directions), ``A``
        (B,N,nx,nx), ``B`` (B,N,nx,nu), ``X`` (B,N+1,nx), ``info`` (B,), ``delta`` (B,).  A
        scenario whose ``info`` is not 0 has NaN in every array.  Equality rows raise
        ``ValueError``, as :meth:`sensitivity_fused` does."""
        N, nu, nx = self._policy_dims()
        d, nd = (None, 0) if dp is None else self._dp_dirs(dp, 0)
        if nd == 0:
            d = None
        ins, B = self._point_ins_host(sol, lbx, ubx, lbg, ubg, p)
        ins.append((None, 0) if d is None else self._dp_arg(d, B)[0])
        K, A, Bm = np.empty((B, N, nx, nu)), np.empty((B, N, nx, nx)), np.empty((B, N, nu, nx))
        kff = np.empty((B, nd, N, nu)) if nd else None
        X = np.empty((B, N + 1, nx))
        info, delta = np.empty(B, dtype=np.int32), np.empty(B)
        _lib.check(_lib.lib().nmpc_solve_policy_batch(
            self._h, B, nd, *_flat_ins(ins), _dptr(K), _dptr(kff) if nd else None, _dptr(A), _dptr(Bm),
            _dptr(X), info.ctypes.data_as(_IP), _dptr(delta)))
        self._raise_equality_rows(info, lbg, ubg, "policy_fused")
        # the blocks are column-major: K_k is stored (nx, nu), A_k (nx, nx), B_k (nu, nx)
        return {"K": np.ascontiguousarray(K.transpose(0, 1, 3, 2)), "kff": kff,
                "A": np.ascontiguousarray(A.transpose(0, 1, 3, 2)), "B": np.ascontiguousarray(Bm.transpose(0, 1, 3, 2)),
                "X": X, "info": info, "delta": delta}

    def policy_device(self, sol: dict, lbx, ubx, lbg, ubg, p, dp=None, out: dict | None = None, stream=None):
        """The feedback policy along the plan (``nmpc_solve_policy_batch_dev``), torch CUDA float64
        tensors in and out: ``sol``, the bounds, ``p`` and ``dp`` ((B,nd,np), shared (nd,np), or
        None for no direction) as :meth:`sensitivity_device` takes them.  Returns a dict of
        ``K`` (B,N,nu,nx), the stage gains; ``kff`` (B,nd,N,nu), the feedforward per direction
        (None without directions); ``A`` (B,N,nx,nx) and ``B`` (B,N,nx,nu), the stage matrices of
        x_{k+1} = x_k + T f(x_k, u_k); ``X`` (B,N+1,nx), the plan's states; ``info`` (B,) int32 and
        ``delta`` (B,).  K, A and B are transposed views of the kernel's column-major blocks.
        ``out`` may hold the raw buffers of an earlier call (the returned dict's ``"raw"``) to
        reuse them.  A scenario whose ``info`` is not 0 has NaN everywhere.  Enqueued on
        ``stream`` (default = current); never synchronises the host and reads nothing back."""
        import torch  # plumbing only: device memory and streams

        N, nu, nx = self._policy_dims()
        ins, B = self._point_ins_device(sol, lbx, ubx, lbg, ubg, p)
        x = sol["x"]
        nd = 0 if dp is None else dp.shape[-2]
        ins += _dev_in(dp if nd else None, (nd, self.np), B, "dp")
        if stream is None:
            stream = torch.cuda.current_stream()
        shapes = {"K": (B, N, nx, nu), "kff": (B, nd, N, nu), "A": (B, N, nx, nx), "B": (B, N, nu, nx),
                  "X": (B, N + 1, nx), "info": (B,), "delta": (B,)}
        raw = {}
        with torch.cuda.stream(stream):
            for k, shp in shapes.items():
                raw[k] = (out or {}).get(k)
                if k == "kff" and nd == 0:
                    raw[k] = None
                elif raw[k] is None:
                    raw[k] = torch.empty(shp, dtype=torch.int32 if k == "info" else torch.float64, device=x.device)
        ptr = _dev_outs(raw, shapes.items())
        _lib.check(_lib.lib().nmpc_solve_policy_batch_dev(self._h, B, nd, *ins, *ptr, _stream_ptr(stream)))
        return {"K": raw["K"].transpose(2, 3), "kff": raw["kff"], "A": raw["A"].transpose(2, 3),
                "B": raw["B"].transpose(2, 3), "X": raw["X"], "info": raw["info"], "delta": raw["delta"], "raw": raw}

    # ---- disturbance rollouts of the policy on the plant (nmpc_policy_rollout_batch)
    ROLLOUT_OUT = ("J", "viol", "nsat", "X", "U")

    def _rollout_shapes(self, B, M):
        N, nu, nx = self._policy_dims()
        return {"J": (B, M), "viol": (B, M), "nsat": (B, M), "X": (B, M, N + 1, nx), "U": (B, M, N, nu)}

    def policy_rollout_device(self, p, ubar, Xbar, K, e0, w=None, lbx=None, ubx=None, lbg=None, ubg=None,
                              out: dict | None = None, want=("J", "viol", "nsat"), stream=None):
        """M disturbance rollouts per scenario of the clamped policy u_k = clamp(ubar_k + K_k (x_k -
        Xbar_k)) on the nonlinear plant (``nmpc_policy_rollout_batch_dev``, whose comment states
        the formula), torch CUDA float64 tensors in and out.  ``p`` (B,np), ``ubar`` (B,nw),
        ``lbx`` / ``ubx`` (B,nw) and ``lbg`` / ``ubg`` (B,ng) may each be shared, (n,); ``Xbar`` is
        (B,N+1,nx) or shared (N+1,nx); ``K`` is :meth:`policy_device`'s gains -- its ``K`` view
        (B,N,nu,nx) or the raw column-major buffer (B,N,nx,nu), or shared without the B -- or None
        for the open-loop replay of ``ubar``; ``e0`` is (B,M,nx) or shared (M,nx), the initial-state
        disturbances, and ``w`` (B,M,N,nx) or (M,N,nx), the process disturbances, or None.  Returns
        a dict with the outputs named in ``want`` and those preallocated in ``out``: ``J`` (B,M),
        ``viol`` (B,M), ``nsat`` (B,M) int32, ``X`` (B,M,N+1,nx), ``U`` (B,M,N,nu).  A NaN in a
        sample's inputs, or in its scenario's policy, gives NaN in that sample's J and viol.
        Enqueued on ``stream`` (default = current); never synchronises the host, reads nothing
        back and uses no workspace of the handle."""
        import torch  # plumbing only: device memory and streams

        N, nu, nx = self._policy_dims()

        assert e0.dim() in (2, 3) and e0.shape[-1] == nx, ("e0", tuple(e0.shape))
        M = e0.shape[-2]
        B = None
        for t, lead in ((e0, 3), (p, 2), (ubar, 2), (Xbar, 3), (w, 4)):
            if t is not None and t.dim() == lead:
                B = t.shape[0]
                break
        if B is None:
            raise ValueError("policy_rollout_device: no argument carries the batch size")

        if K is not None and tuple(K.shape[-2:]) == (nu, nx):
            K = K.transpose(-1, -2)  # policy_device's view back to the kernel's column-major blocks
        if p is None or ubar is None or Xbar is None:
            raise ValueError("p, ubar and Xbar are required")
        if (lbg is None) != (ubg is None):
            raise ValueError("lbg and ubg must be given together")
        ins = _dev_ins((("p", p, (self.np,)), ("ubar", ubar, (self.nw,)), ("Xbar", Xbar, (N + 1, nx)),
                        ("K", K, (N, nx, nu)), ("lbx", lbx, (self.nw,)), ("ubx", ubx, (self.nw,)),
                        ("lbg", lbg, (self.ng,)), ("ubg", ubg, (self.ng,)), ("e0", e0, (M, nx)),
                        ("w", w, (M, N, nx))), B)
        if stream is None:
            stream = torch.cuda.current_stream()
        shapes = self._rollout_shapes(B, M)
        res = dict(out or {})
        with torch.cuda.stream(stream):
            for k in want:
                if res.get(k) is None:
                    res[k] = torch.empty(shapes[k], dtype=torch.int32 if k == "nsat" else torch.float64,
                                         device=e0.device)
        if all(res.get(k) is None for k in ("J", "viol", "X", "U")):
            raise ValueError("policy_rollout_device: one of J, viol, X, U is required")
        ptr = _dev_outs(res, shapes.items())
        _lib.check(_lib.lib().nmpc_policy_rollout_batch_dev(self._h, B, M, *ins, *ptr, _stream_ptr(stream)))
        return {k: v for k, v in res.items() if v is not None}

    def policy_rollout(self, p, ubar, Xbar, K, e0, w=None, lbx=None, ubx=None, lbg=None, ubg=None,
                       want=("J", "viol", "nsat", "X", "U")):
        """:meth:`policy_rollout_device` through the host entry point
        (``nmpc_policy_rollout_batch``), NumPy arrays in the same scenario-major shapes: ``p``
        (B,np), ``ubar`` (B,nw), ``Xbar`` (B,N+1,nx), ``K`` (B,N,nu,nx) (row-major blocks, as
        :meth:`policy_fused` returns them) or None, ``e0`` (B,M,nx), ``w`` (B,M,N,nx) or None, the
        bounds (B,n) -- each may be shared (without the B).  Returns the outputs named in ``want``."""
        N, nu, nx = self._policy_dims()
        e0 = np.ascontiguousarray(e0, dtype=np.float64)
        if e0.ndim not in (2, 3) or e0.shape[-1] != nx:
            raise ValueError(f"e0: expected (M,{nx}) or (B,M,{nx}), got shape {e0.shape}")
        M = e0.shape[-2]
        if K is not None:
            K = np.asarray(K, dtype=np.float64)
            if K.shape[-2:] != (nu, nx):
                raise ValueError(f"K: expected blocks of ({nu},{nx}), got shape {K.shape}")
            K = np.swapaxes(K, -1, -2)  # to the kernel's column-major blocks
        fields = (("p", p, (self.np,)), ("ubar", ubar, (self.nw,)), ("Xbar", Xbar, (N + 1, nx)), ("K", K, (N, nx, nu)),
                  ("lbx", lbx, (self.nw,)), ("ubx", ubx, (self.nw,)), ("lbg", lbg, (self.ng,)), ("ubg", ubg, (self.ng,)),
                  ("e0", e0, (M, nx)), ("w", w, (M, N, nx)))
        arrs, B = [], None
        for name, a, tail in fields:
            if a is None:
                if name in ("p", "ubar", "Xbar"):
                    raise ValueError(f"{name} is required")
                arrs.append((None, 0))
                continue
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.shape == tail:
                arrs.append((a, 0))
                continue
            if a.shape[1:] != tail or B not in (None, a.shape[0]):
                raise ValueError(f"{name}: expected {tail} or (B,) + {tail}, got shape {a.shape}")
            B = a.shape[0]
            arrs.append((a, int(np.prod(tail))))
        if B is None:
            raise ValueError("policy_rollout: no argument carries the batch size")
        if (lbg is None) != (ubg is None):
            raise ValueError("lbg and ubg must be given together")
        shapes = self._rollout_shapes(B, M)
        res = {k: np.empty(shapes[k], dtype=np.int32 if k == "nsat" else np.float64) for k in self.ROLLOUT_OUT
               if k in want}
        if not any(k in res for k in ("J", "viol", "X", "U")):
            raise ValueError("policy_rollout: one of J, viol, X, U is required")
        ptr = [None if k not in res else (res[k].ctypes.data_as(_IP) if k == "nsat" else _dptr(res[k]))
               for k in self.ROLLOUT_OUT]
        _lib.check(_lib.lib().nmpc_policy_rollout_batch(self._h, B, M, *_flat_ins(arrs), *ptr))
        return res

    # ---- the reverse sweep of those rollouts (nmpc_policy_rollout_adjoint_batch)
    ROLLOUT_ADJ_OUT = ("ubar_bar", "K_bar", "Xbar_bar", "p_bar", "e0_bar", "w_bar", "nsat")

    def _rollout_adjoint_shapes(self, B, M):
        N, nu, nx = self._policy_dims()
        return {"ubar_bar": (B, self.nw), "K_bar": (B, N, nx, nu), "Xbar_bar": (B, N + 1, nx), "p_bar": (B, self.np),
                "e0_bar": (B, M, nx), "w_bar": (B, M, N, nx), "nsat": (B, M)}

    def policy_rollout_adjoint_device(self, p, ubar, Xbar, K, X, Jb=None, Xb=None, Ub=None, lbx=None, ubx=None,
                                      out: dict | None = None, want=("ubar_bar", "p_bar"), stream=None):
        """The reverse sweep of :meth:`policy_rollout_device` at its trajectories ``X`` (B,M,N+1,nx)
        (``nmpc_policy_rollout_adjoint_batch_dev``, whose comment states the recursion): the gradient
        of sum_s (Jb_s J_s + <Xb_s, X_s> + <Ub_s, U_s>) per scenario, torch CUDA float64 tensors in
        and out.  ``p``, ``ubar``, ``Xbar``, ``K``, ``lbx`` and ``ubx`` are the forward call's; the
        seeds ``Jb`` (B,M), ``Xb`` (B,M,N+1,nx) and ``Ub`` (B,M,N,nu) may each be None or shared
        (without the B), one at least is required.  Returns a dict with the outputs named in
        ``want`` and those preallocated in ``out``: ``ubar_bar`` (B,nw), ``K_bar`` (B,N,nx,nu) -- the
        kernel's column-major blocks, the layout of :meth:`policy_device`'s raw ``K`` --,
        ``Xbar_bar`` (B,N+1,nx) and ``p_bar`` (B,np), summed over the M samples; ``e0_bar`` (B,M,nx)
        and ``w_bar`` (B,M,N,nx) per sample; ``nsat`` (B,M) int32, recounted.  ``K_bar`` and
        ``Xbar_bar`` need ``K``.  Enqueued on ``stream`` (default = current); never synchronises the
        host and reads nothing back; uses the handle's workspace only when M > 64."""
        import torch  # plumbing only: device memory and streams

        N, nu, nx = self._policy_dims()
        assert X.dim() in (3, 4) and tuple(X.shape[-2:]) == (N + 1, nx), ("X", tuple(X.shape))
        M = X.shape[-3]
        B = None
        for t, lead in ((X, 4), (p, 2), (ubar, 2), (Xbar, 3), (Jb, 2), (Xb, 4), (Ub, 4)):
            if t is not None and t.dim() == lead:
                B = t.shape[0]
                break
        if B is None:
            raise ValueError("policy_rollout_adjoint_device: no argument carries the batch size")
        if K is not None and tuple(K.shape[-2:]) == (nu, nx):
            K = K.transpose(-1, -2)  # policy_device's view back to the kernel's column-major blocks
        if p is None or ubar is None or Xbar is None:
            raise ValueError("p, ubar and Xbar are required")
        if Jb is None and Xb is None and Ub is None:
            raise ValueError("policy_rollout_adjoint_device: one of the seeds Jb, Xb, Ub is required")
        ins = _dev_ins((("p", p, (self.np,)), ("ubar", ubar, (self.nw,)), ("Xbar", Xbar, (N + 1, nx)),
                        ("K", K, (N, nx, nu)), ("lbx", lbx, (self.nw,)), ("ubx", ubx, (self.nw,)),
                        ("X", X, (M, N + 1, nx)), ("Jb", Jb, (M,)), ("Xb", Xb, (M, N + 1, nx)),
                        ("Ub", Ub, (M, N, nu))), B)
        if stream is None:
            stream = torch.cuda.current_stream()
        shapes = self._rollout_adjoint_shapes(B, M)
        res = dict(out or {})
        with torch.cuda.stream(stream):
            for k in want:
                if res.get(k) is None:
                    res[k] = torch.empty(shapes[k], dtype=torch.int32 if k == "nsat" else torch.float64,
                                         device=X.device)
        if all(res.get(k) is None for k in self.ROLLOUT_ADJ_OUT[:6]):
            raise ValueError("policy_rollout_adjoint_device: one of " + ", ".join(self.ROLLOUT_ADJ_OUT[:6])
                             + " is required")
        if K is None and (res.get("K_bar") is not None or res.get("Xbar_bar") is not None):
            raise ValueError("policy_rollout_adjoint_device: K_bar and Xbar_bar need K")
        ptr = _dev_outs(res, [(k, shapes[k]) for k in self.ROLLOUT_ADJ_OUT])
        _lib.check(_lib.lib().nmpc_policy_rollout_adjoint_batch_dev(self._h, B, M, *ins, *ptr, _stream_ptr(stream)))
        return {k: v for k, v in res.items() if v is not None}

    def policy_rollout_adjoint(self, p, ubar, Xbar, K, X, Jb=None, Xb=None, Ub=None, lbx=None, ubx=None,
                               want=("ubar_bar", "K_bar", "Xbar_bar", "p_bar", "e0_bar", "w_bar", "nsat")):
        """:meth:`policy_rollout_adjoint_device` through the host entry point
        (``nmpc_policy_rollout_adjoint_batch``), NumPy arrays in the same scenario-major shapes;
        ``K`` (B,N,nu,nx) in row-major blocks, as :meth:`policy_fused` returns them, or None, and
        ``K_bar`` (B,N,nu,nx) likewise.  Each input may be shared (without the B).  Returns
        the outputs named in ``want`` (``K_bar`` and ``Xbar_bar`` are left out when K is None)."""
        N, nu, nx = self._policy_dims()
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.ndim not in (3, 4) or X.shape[-2:] != (N + 1, nx):
            raise ValueError(f"X: expected (M,{N + 1},{nx}) or (B,M,{N + 1},{nx}), got shape {X.shape}")
        M = X.shape[-3]
        if K is not None:
            K = np.asarray(K, dtype=np.float64)
            if K.shape[-2:] != (nu, nx):
                raise ValueError(f"K: expected blocks of ({nu},{nx}), got shape {K.shape}")
            K = np.swapaxes(K, -1, -2)  # to the kernel's column-major blocks
        fields = (("p", p, (self.np,)), ("ubar", ubar, (self.nw,)), ("Xbar", Xbar, (N + 1, nx)), ("K", K, (N, nx, nu)),
                  ("lbx", lbx, (self.nw,)), ("ubx", ubx, (self.nw,)), ("X", X, (M, N + 1, nx)), ("Jb", Jb, (M,)),
                  ("Xb", Xb, (M, N + 1, nx)), ("Ub", Ub, (M, N, nu)))
        arrs, B = [], None
        for name, a, tail in fields:
            if a is None:
                if name in ("p", "ubar", "Xbar"):
                    raise ValueError(f"{name} is required")
                arrs.append((None, 0))
                continue
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.shape == tail:
                arrs.append((a, 0))
                continue
            if a.shape[1:] != tail or B not in (None, a.shape[0]):
                raise ValueError(f"{name}: expected {tail} or (B,) + {tail}, got shape {a.shape}")
            B = a.shape[0]
            arrs.append((a, int(np.prod(tail))))
        if B is None:
            raise ValueError("policy_rollout_adjoint: no argument carries the batch size")
        if Jb is None and Xb is None and Ub is None:
            raise ValueError("policy_rollout_adjoint: one of the seeds Jb, Xb, Ub is required")
        shapes = self._rollout_adjoint_shapes(B, M)
        res = {k: np.empty(shapes[k], dtype=np.int32 if k == "nsat" else np.float64) for k in self.ROLLOUT_ADJ_OUT
               if k in want and not (K is None and k in ("K_bar", "Xbar_bar"))}
        if not any(k in res for k in self.ROLLOUT_ADJ_OUT[:6]):
            raise ValueError("policy_rollout_adjoint: one of " + ", ".join(self.ROLLOUT_ADJ_OUT[:6]) + " is required")
        ptr = [None if k not in res else (res[k].ctypes.data_as(_IP) if k == "nsat" else _dptr(res[k]))
               for k in self.ROLLOUT_ADJ_OUT]
        _lib.check(_lib.lib().nmpc_policy_rollout_adjoint_batch(self._h, B, M, *_flat_ins(arrs), *ptr))
        if "K_bar" in res:
            res["K_bar"] = np.ascontiguousarray(np.swapaxes(res["K_bar"], -1, -2))
        return res

    # ---- the policy's cost-to-go expansion: expected cost and its variance
    # (nmpc_policy_value_batch)
    VALUE_OUT = ("J", "lam", "P", "dJ", "varJ")

    def _value_shapes(self, B, nc):
        N, nu, nx = self._policy_dims()
        return {"J": (B,), "lam": (B, N + 1, nx), "P": (B, N + 1, nx, nx), "dJ": (B, nc), "varJ": (B, nc)}

    def policy_value_device(self, p, ubar, Xbar, K, S0=None, W=None, out: dict | None = None,
                            want=("J", "dJ", "varJ"), stream=None):
        """The local quadratic model of the closed loop's cost-to-go along the plan under the unclamped
        policy u_k = ubar_k + K_k (x_k - Xbar_k), and from it the expected cost and its variance
        (``nmpc_policy_value_batch_dev``, whose comment states the recursion), torch CUDA float64
        tensors in and out.  ``p``, ``ubar``, ``Xbar``, ``K``, ``S0`` and ``W`` as
        :meth:`policy_covariance_device` takes them (``K`` None: open loop; ``S0`` None: nc = 0, no
        cases).  Returns a dict with the outputs named in ``want`` and those preallocated in ``out``:
        ``J`` (B,) the plan's cost, ``lam`` (B,N+1,nx) and ``P`` (B,N+1,nx,nx) the gradient and the
        exactly symmetric Hessian of the cost-to-go at every stage (stage N's are 0), ``dJ`` (B,nc) with
        E[J] = J + dJ to second order and ``varJ`` (B,nc) the variance of J to first order; without
        cases ``dJ`` and ``varJ`` are left out.  Enqueued on ``stream`` (default = current); never
        synchronises the host and reads nothing back; the handle's workspace serves, grown only when
        it does not cover B scenarios yet (a solve's does)."""
        import torch  # plumbing only: device memory and streams

        N, nu, nx = self._policy_dims()
        if p is None or ubar is None or Xbar is None:
            raise ValueError("p, ubar and Xbar are required")
        if S0 is None and W is not None:
            raise ValueError("W needs S0")
        nc = 0
        if S0 is not None:
            assert S0.dim() in (3, 4) and tuple(S0.shape[-2:]) == (nx, nx), ("S0", tuple(S0.shape))
            nc = S0.shape[-3]
        B = None
        for t, lead in ((S0, 4), (p, 2), (ubar, 2), (Xbar, 3), (W, 4), (K, 4)):
            if t is not None and t.dim() == lead:
                B = t.shape[0]
                break
        if B is None:
            raise ValueError("policy_value_device: no argument carries the batch size")
        if K is not None and tuple(K.shape[-2:]) == (nu, nx):
            K = K.transpose(-1, -2)  # policy_device's view back to the kernel's column-major blocks
        ins = _dev_ins((("p", p, (self.np,)), ("ubar", ubar, (self.nw,)), ("Xbar", Xbar, (N + 1, nx)),
                        ("K", K, (N, nx, nu)), ("S0", S0, (nc, nx, nx)), ("W", W, (nc, nx, nx))), B)
        if stream is None:
            stream = torch.cuda.current_stream()
        shapes = self._value_shapes(B, nc)
        res = dict(out or {})
        with torch.cuda.stream(stream):
            for k in want:
                if res.get(k) is None and not (nc == 0 and k in ("dJ", "varJ")):
                    res[k] = torch.empty(shapes[k], dtype=torch.float64, device=Xbar.device)
        if all(res.get(k) is None for k in self.VALUE_OUT):
            raise ValueError("policy_value_device: one of " + ", ".join(self.VALUE_OUT) + " is required")
        ptr = _dev_outs(res, shapes.items())
        _lib.check(_lib.lib().nmpc_policy_value_batch_dev(self._h, B, nc, *ins, *ptr, _stream_ptr(stream)))
        return {k: v for k, v in res.items() if v is not None}

    def policy_value(self, p, ubar, Xbar, K, S0=None, W=None, want=("J", "lam", "P", "dJ", "varJ")):
        """:meth:`policy_value_device` through the host entry point (``nmpc_policy_value_batch``),
        NumPy arrays in the same scenario-major shapes as :meth:`policy_covariance` takes them: ``K``
        (B,N,nu,nx) (row-major blocks) or None, ``S0`` (B,nc,nx,nx) or None (no cases) and ``W`` --
        each may be shared (without the B).  Returns the outputs named in ``want``."""
        N, nu, nx = self._policy_dims()
        nc = 0
        if S0 is not None:
            S0 = np.ascontiguousarray(S0, dtype=np.float64)
            if S0.ndim not in (3, 4) or S0.shape[-2:] != (nx, nx):
                raise ValueError(f"S0: expected (nc,{nx},{nx}) or (B,nc,{nx},{nx}), got shape {S0.shape}")
            nc = S0.shape[-3]
        elif W is not None:
            raise ValueError("W needs S0")
        if K is not None:
            K = np.asarray(K, dtype=np.float64)
            if K.shape[-2:] != (nu, nx):
                raise ValueError(f"K: expected blocks of ({nu},{nx}), got shape {K.shape}")
            K = np.swapaxes(K, -1, -2)  # to the kernel's column-major blocks
        fields = (("p", p, (self.np,)), ("ubar", ubar, (self.nw,)), ("Xbar", Xbar, (N + 1, nx)), ("K", K, (N, nx, nu)),
                  ("S0", S0, (nc, nx, nx)), ("W", W, (nc, nx, nx)))
        arrs, B = [], None
        for name, a, tail in fields:
            if a is None:
                if name in ("p", "ubar", "Xbar"):
                    raise ValueError(f"{name} is required")
                arrs.append((None, 0))
                continue
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.shape == tail:
                arrs.append((a, 0))
                continue
            if a.shape[1:] != tail or B not in (None, a.shape[0]):
                raise ValueError(f"{name}: expected {tail} or (B,) + {tail}, got shape {a.shape}")
            B = a.shape[0]
            arrs.append((a, int(np.prod(tail))))
        if B is None:
            raise ValueError("policy_value: no argument carries the batch size")
        shapes = self._value_shapes(B, nc)
        res = {k: np.empty(shapes[k]) for k in self.VALUE_OUT if k in want and not (nc == 0 and k in ("dJ", "varJ"))}
        if not res:
            raise ValueError("policy_value: one of " + ", ".join(self.VALUE_OUT) + " is required")
        ptr = [_dptr(res[k]) if k in res else None for k in self.VALUE_OUT]
        _lib.check(_lib.lib().nmpc_policy_value_batch(self._h, B, nc, *_flat_ins(arrs), *ptr))
        return res

    # ---- the policy's closed-loop covariance and the rows' standard deviations
    # (nmpc_policy_covariance_batch)
    COVARIANCE_OUT = ("Sigma", "sigma_u", "sigma_g")

    def _covariance_shapes(self, B, nc):
        N, nu, nx = self._policy_dims()
        return {"Sigma": (B, nc, N + 1, nx, nx), "sigma_u": (B, nc, N, nu), "sigma_g": (B, nc, N + 1, self.ng // (N + 1))}

    def policy_covariance_device(self, p, ubar, Xbar, K, S0, W=None, obs_var=None, out: dict | None = None,
                                 want=("sigma_g", "sigma_u"), stream=None):
        """The state covariance around the plan under the policy u_k = ubar_k + K_k (x_k - Xbar_k),
        Sigma_{k+1} = (A_k + B_k K_k) Sigma_k (A_k + B_k K_k)^T + W from Sigma_0 = S0, and the standard
        deviations of every control and every row (``nmpc_policy_covariance_batch_dev``, whose comment
        states the recursion), torch CUDA float64 tensors in and out.  ``p``, ``ubar``, ``Xbar`` and ``K``
        as :meth:`policy_rollout_device` takes them (``K`` None: open loop).  ``S0`` is (B,nc,nx,nx)
        or shared (nc,nx,nx), one initial covariance per case, and ``W`` likewise or None, the process
        noise added at every stage; the blocks are column-major, entry (i, j) at ``[..., j, i]``, and
        only the entries with i >= j are read (a symmetric matrix is passed as it is).  ``obs_var``
        (B,n_obs) or (n_obs,) or None is the isotropic variance of each obstacle's centre.  Returns a
        dict with the outputs named in ``want`` and those preallocated in ``out``: ``Sigma``
        (B,nc,N+1,nx,nx), exactly symmetric; ``sigma_u`` (B,nc,N,nu); ``sigma_g`` (B,nc,N+1,m), stage 0's
        rows at S0.  The kernel knows nothing about clamps: zero a control's row of K where it is held on
        its bound.  Enqueued on ``stream`` (default = current); never synchronises the host, reads
        nothing back and uses no workspace of the handle."""
        import torch  # plumbing only: device memory and streams

        N, nu, nx = self._policy_dims()
        if p is None or ubar is None or Xbar is None or S0 is None:
            raise ValueError("p, ubar, Xbar and S0 are required")
        assert S0.dim() in (3, 4) and tuple(S0.shape[-2:]) == (nx, nx), ("S0", tuple(S0.shape))
        nc = S0.shape[-3]
        B = None
        for t, lead in ((S0, 4), (p, 2), (ubar, 2), (Xbar, 3), (W, 4), (obs_var, 2)):
            if t is not None and t.dim() == lead:
                B = t.shape[0]
                break
        if B is None:
            raise ValueError("policy_covariance_device: no argument carries the batch size")
        if K is not None and tuple(K.shape[-2:]) == (nu, nx):
            K = K.transpose(-1, -2)  # policy_device's view back to the kernel's column-major blocks
        ins = _dev_ins((("p", p, (self.np,)), ("ubar", ubar, (self.nw,)), ("Xbar", Xbar, (N + 1, nx)),
                        ("K", K, (N, nx, nu)), ("S0", S0, (nc, nx, nx)), ("W", W, (nc, nx, nx)),
                        ("obs_var", obs_var, (self.spec.n_obs,))), B)
        if stream is None:
            stream = torch.cuda.current_stream()
        shapes = self._covariance_shapes(B, nc)
        res = dict(out or {})
        with torch.cuda.stream(stream):
            for k in want:
                if res.get(k) is None:
                    res[k] = torch.empty(shapes[k], dtype=torch.float64, device=S0.device)
        if all(res.get(k) is None for k in self.COVARIANCE_OUT):
            raise ValueError("policy_covariance_device: one of Sigma, sigma_u, sigma_g is required")
        ptr = _dev_outs(res, shapes.items())
        _lib.check(_lib.lib().nmpc_policy_covariance_batch_dev(self._h, B, nc, *ins, *ptr, _stream_ptr(stream)))
        return {k: v for k, v in res.items() if v is not None}

    def policy_covariance(self, p, ubar, Xbar, K, S0, W=None, obs_var=None, want=("Sigma", "sigma_u", "sigma_g")):
        """:meth:`policy_covariance_device` through the host entry point
        (``nmpc_policy_covariance_batch``), NumPy arrays in the same scenario-major shapes: ``p``
        (B,np), ``ubar`` (B,nw), ``Xbar`` (B,N+1,nx), ``K`` (B,N,nu,nx) (row-major blocks, as
        :meth:`policy_fused` returns them) or None, ``S0`` (B,nc,nx,nx) and ``W`` (column-major
        blocks, entries i >= j read: a symmetric matrix as it is), ``obs_var`` (B,n_obs) -- each may be
        shared (without the B).  Returns the outputs named in ``want``."""
        N, nu, nx = self._policy_dims()
        if S0 is None:
            raise ValueError("S0 is required")
        S0 = np.ascontiguousarray(S0, dtype=np.float64)
        if S0.ndim not in (3, 4) or S0.shape[-2:] != (nx, nx):
            raise ValueError(f"S0: expected (nc,{nx},{nx}) or (B,nc,{nx},{nx}), got shape {S0.shape}")
        nc = S0.shape[-3]
        if K is not None:
            K = np.asarray(K, dtype=np.float64)
            if K.shape[-2:] != (nu, nx):
                raise ValueError(f"K: expected blocks of ({nu},{nx}), got shape {K.shape}")
            K = np.swapaxes(K, -1, -2)  # to the kernel's column-major blocks
        fields = (("p", p, (self.np,)), ("ubar", ubar, (self.nw,)), ("Xbar", Xbar, (N + 1, nx)), ("K", K, (N, nx, nu)),
                  ("S0", S0, (nc, nx, nx)), ("W", W, (nc, nx, nx)), ("obs_var", obs_var, (self.spec.n_obs,)))
        arrs, B = [], None
        for name, a, tail in fields:
            if a is None:
                if name in ("p", "ubar", "Xbar"):
                    raise ValueError(f"{name} is required")
                arrs.append((None, 0))
                continue
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.shape == tail:
                arrs.append((a, 0))
                continue
            if a.shape[1:] != tail or B not in (None, a.shape[0]):
                raise ValueError(f"{name}: expected {tail} or (B,) + {tail}, got shape {a.shape}")
            B = a.shape[0]
            arrs.append((a, int(np.prod(tail))))
        if B is None:
            raise ValueError("policy_covariance: no argument carries the batch size")
        shapes = self._covariance_shapes(B, nc)
        res = {k: np.empty(shapes[k]) for k in self.COVARIANCE_OUT if k in want}
        if not res:
            raise ValueError("policy_covariance: one of Sigma, sigma_u, sigma_g is required")
        ptr = [_dptr(res[k]) if k in res else None for k in self.COVARIANCE_OUT]
        _lib.check(_lib.lib().nmpc_policy_covariance_batch(self._h, B, nc, *_flat_ins(arrs), *ptr))
        return res

    # ---- the reverse sweep of that covariance (nmpc_policy_covariance_adjoint_batch)
    COVARIANCE_ADJ_OUT = ("S0_bar", "W_bar", "Lambda", "obs_var_bar", "K_bar", "ubar_bar", "Xbar_bar", "p_bar")

    def _covariance_adjoint_shapes(self, B, nc):
        N, nu, nx = self._policy_dims()
        return {"S0_bar": (B, nc, nx, nx), "W_bar": (B, nc, nx, nx), "Lambda": (B, nc, N + 1, nx, nx),
                "obs_var_bar": (B, nc, self.spec.n_obs), "K_bar": (B, nc, N, nx, nu), "ubar_bar": (B, nc, self.nw),
                "Xbar_bar": (B, nc, N + 1, nx), "p_bar": (B, nc, self.np)}

    def policy_covariance_adjoint_device(self, p, ubar, Xbar, K, Sigma, Sigma_bar=None, var_u_bar=None,
                                         var_g_bar=None, out: dict | None = None,
                                         want=("S0_bar", "K_bar", "ubar_bar", "Xbar_bar", "p_bar"), stream=None):
        """The reverse sweep of :meth:`policy_covariance_device` at its ``Sigma`` (B,nc,N+1,nx,nx)
        (``nmpc_policy_covariance_adjoint_batch_dev``, whose comment states the recursion): the
        gradient of sum_k <Sigma_bar_k, Sigma_k> + <var_u_bar, sigma_u^2> + <var_g_bar, sigma_g^2> per
        (scenario, case), torch CUDA float64 tensors in and out.  ``p``, ``ubar``, ``Xbar`` and ``K`` are
        the forward call's (``K`` also in :meth:`policy_device`'s (…,nu,nx) view).  The seeds
        ``Sigma_bar`` (B,nc,N+1,nx,nx) -- any blocks, symmetrised by the kernel --, ``var_u_bar``
        (B,nc,N,nu) and ``var_g_bar`` (B,nc,N+1,m) are on the VARIANCES, may each be None or shared
        (without the B), and one at least is required.  Returns a dict with the outputs named in
        ``want`` and those preallocated in ``out``, each per (scenario, case): ``S0_bar`` and ``W_bar``
        (B,nc,nx,nx), exactly symmetric; ``Lambda`` (B,nc,N+1,nx,nx), the gradient with respect to a
        covariance injected at each stage; ``obs_var_bar`` (B,nc,n_obs); ``K_bar`` (B,nc,N,nx,nu), the
        kernel's column-major blocks (needs ``K``); ``ubar_bar`` (B,nc,nw); ``Xbar_bar`` (B,nc,N+1,nx);
        ``p_bar`` (B,nc,np), 0 outside the obstacle centres taken from p.  A caller whose input is
        shared by the cases or the scenarios sums.  Enqueued on ``stream`` (default = current); never
        synchronises the host, reads nothing back and uses no workspace of the handle."""
        import torch  # plumbing only: device memory and streams

        N, nu, nx = self._policy_dims()
        m = self.ng // (N + 1)
        if p is None or ubar is None or Xbar is None or Sigma is None:
            raise ValueError("p, ubar, Xbar and Sigma are required")
        assert Sigma.dim() in (4, 5) and tuple(Sigma.shape[-3:]) == (N + 1, nx, nx), ("Sigma", tuple(Sigma.shape))
        nc = Sigma.shape[-4]
        B = None
        for t, lead in ((Sigma, 5), (p, 2), (ubar, 2), (Xbar, 3), (Sigma_bar, 5), (var_u_bar, 4), (var_g_bar, 4)):
            if t is not None and t.dim() == lead:
                B = t.shape[0]
                break
        if B is None:
            raise ValueError("policy_covariance_adjoint_device: no argument carries the batch size")
        if Sigma_bar is None and var_u_bar is None and var_g_bar is None:
            raise ValueError("policy_covariance_adjoint_device: one of the seeds Sigma_bar, var_u_bar, var_g_bar "
                             "is required")
        if K is not None and tuple(K.shape[-2:]) == (nu, nx):
            K = K.transpose(-1, -2)  # policy_device's view back to the kernel's column-major blocks
        ins = _dev_ins((("p", p, (self.np,)), ("ubar", ubar, (self.nw,)), ("Xbar", Xbar, (N + 1, nx)),
                        ("K", K, (N, nx, nu)), ("Sigma", Sigma, (nc, N + 1, nx, nx)),
                        ("Sigma_bar", Sigma_bar, (nc, N + 1, nx, nx)), ("var_u_bar", var_u_bar, (nc, N, nu)),
                        ("var_g_bar", var_g_bar, (nc, N + 1, m))), B)
        if stream is None:
            stream = torch.cuda.current_stream()
        shapes = self._covariance_adjoint_shapes(B, nc)
        res = dict(out or {})
        with torch.cuda.stream(stream):
            for k in want:
                if res.get(k) is None:
                    res[k] = torch.empty(shapes[k], dtype=torch.float64, device=Sigma.device)
        if all(res.get(k) is None for k in self.COVARIANCE_ADJ_OUT):
            raise ValueError("policy_covariance_adjoint_device: one of " + ", ".join(self.COVARIANCE_ADJ_OUT)
                             + " is required")
        if K is None and res.get("K_bar") is not None:
            raise ValueError("policy_covariance_adjoint_device: K_bar needs K")
        ptr = _dev_outs(res, [(k, shapes[k]) for k in self.COVARIANCE_ADJ_OUT])
        _lib.check(_lib.lib().nmpc_policy_covariance_adjoint_batch_dev(self._h, B, nc, *ins, *ptr, _stream_ptr(stream)))
        return {k: v for k, v in res.items() if v is not None}

    def policy_covariance_adjoint(self, p, ubar, Xbar, K, Sigma, Sigma_bar=None, var_u_bar=None, var_g_bar=None,
                                  want=COVARIANCE_ADJ_OUT):
        """:meth:`policy_covariance_adjoint_device` through the host entry point
        (``nmpc_policy_covariance_adjoint_batch``), NumPy arrays in the same scenario-major shapes;
        ``K`` (B,N,nu,nx) in row-major blocks, as :meth:`policy_fused` returns them, or None, and
        ``K_bar`` (B,nc,N,nu,nx) likewise.  Each input may be shared (without the B).  Returns the
        outputs named in ``want`` (``K_bar`` is left out when K is None, ``obs_var_bar`` when the
        problem has no obstacles)."""
        N, nu, nx = self._policy_dims()
        m = self.ng // (N + 1)
        if Sigma is None:
            raise ValueError("Sigma is required")
        Sigma = np.ascontiguousarray(Sigma, dtype=np.float64)
        if Sigma.ndim not in (4, 5) or Sigma.shape[-3:] != (N + 1, nx, nx):
            raise ValueError(f"Sigma: expected (nc,{N + 1},{nx},{nx}) or (B,nc,{N + 1},{nx},{nx}), got shape {Sigma.shape}")
        nc = Sigma.shape[-4]
        if K is not None:
            K = np.asarray(K, dtype=np.float64)
            if K.shape[-2:] != (nu, nx):
                raise ValueError(f"K: expected blocks of ({nu},{nx}), got shape {K.shape}")
            K = np.swapaxes(K, -1, -2)  # to the kernel's column-major blocks
        fields = (("p", p, (self.np,)), ("ubar", ubar, (self.nw,)), ("Xbar", Xbar, (N + 1, nx)), ("K", K, (N, nx, nu)),
                  ("Sigma", Sigma, (nc, N + 1, nx, nx)), ("Sigma_bar", Sigma_bar, (nc, N + 1, nx, nx)),
                  ("var_u_bar", var_u_bar, (nc, N, nu)), ("var_g_bar", var_g_bar, (nc, N + 1, m)))
        arrs, B = [], None
        for name, a, tail in fields:
            if a is None:
                if name in ("p", "ubar", "Xbar"):
                    raise ValueError(f"{name} is required")
                arrs.append((None, 0))
                continue
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.shape == tail:
                arrs.append((a, 0))
                continue
            if a.shape[1:] != tail or B not in (None, a.shape[0]):
                raise ValueError(f"{name}: expected {tail} or (B,) + {tail}, got shape {a.shape}")
            B = a.shape[0]
            arrs.append((a, int(np.prod(tail))))
        if B is None:
            raise ValueError("policy_covariance_adjoint: no argument carries the batch size")
        if Sigma_bar is None and var_u_bar is None and var_g_bar is None:
            raise ValueError("policy_covariance_adjoint: one of the seeds Sigma_bar, var_u_bar, var_g_bar is required")
        shapes = self._covariance_adjoint_shapes(B, nc)
        res = {k: np.empty(shapes[k]) for k in self.COVARIANCE_ADJ_OUT
               if k in want and not (K is None and k == "K_bar") and not (self.spec.n_obs == 0 and k == "obs_var_bar")}
        if not res:
            raise ValueError("policy_covariance_adjoint: one of " + ", ".join(self.COVARIANCE_ADJ_OUT) + " is required")
        ptr = [_dptr(res[k]) if k in res else None for k in self.COVARIANCE_ADJ_OUT]
        _lib.check(_lib.lib().nmpc_policy_covariance_adjoint_batch(self._h, B, nc, *_flat_ins(arrs), *ptr))
        if "K_bar" in res:
            res["K_bar"] = np.ascontiguousarray(np.swapaxes(res["K_bar"], -1, -2))
        return res

    def shift_device(self, p, u_sol, w_out, v_t, w_t, stream=None):
        """Closed-loop shift on device (Python/NMPC_TT.py:13-30), see nmpc_shift_dev."""
        import torch

        L = _lib.lib()
        B = u_sol.shape[0]
        if stream is None:
            stream = torch.cuda.current_stream()
        _lib.check(L.nmpc_shift_dev(self._h, B, C.c_void_p(p.data_ptr()), p.shape[1],
                                    C.c_void_p(u_sol.data_ptr()), C.c_void_p(w_out.data_ptr()),
                                    C.c_void_p(v_t.data_ptr()), C.c_void_p(w_t.data_ptr()),
                                    C.c_void_p(stream.cuda_stream)))

    def closed_loop_device(self, K: int, lbx, ubx, lbg, ubg, p, w, v_t, w_t, hist: dict | None = None,
                           stream=None, p_step=None, order=None, check: bool = True, _validate_order: bool = True):
        """K closed-loop MPC steps per scenario in one launch (see nmpc_closed_loop_dev).

        p (B,np) and w (B,nw) are advanced in place.  Target controls v_t, w_t:
        (B,) per scenario, (1,) shared, (K,1) one schedule for all scenarios
        (targets.schedule), or (K,B).  ``hist`` may hold device tensors
        u (K,B,6), x (K,B,8), f (K,B), fov (K,B), status/iters (K,B) int32.
        ``p_step`` (K,np), optional: added to p[11:] after each step (moving
        obstacles, targets.obstacle_steps).
        ``order`` (B,) int32 device tensor, optional: dispatch order, a permutation
        of range(B) (schedule.longest_first); results do not depend on it.  Validated
        (ValueError) when ``check`` is set; with ``check=False`` a non-permutation is
        reported by check_closed_loop instead.
        ``check`` (default): synchronise and raise unless every scenario completed its K
        steps (check_closed_loop); pass False to stay asynchronous and call
        check_closed_loop later.
        ``_validate_order=False`` (tests only) hands a non-permutation to the device, whose
        completion guard must then report the scenarios it leaves unrun.
        """
        import torch

        L = _lib.lib()
        B = w.shape[0]
        hist = hist or {}
        ins = _dev_ins((("lbx", lbx, (self.nw,)), ("ubx", ubx, (self.nw,)), ("lbg", lbg, (self.ng,)),
                        ("ubg", ubg, (self.ng,))), B)
        assert p.shape == (B, self.np) and p.is_contiguous() and p.dtype == torch.float64
        assert w.shape == (B, self.nw) and w.is_contiguous() and w.dtype == torch.float64
        assert v_t.shape == w_t.shape and v_t.dtype == torch.float64 and w_t.dtype == torch.float64
        assert v_t.is_contiguous() and w_t.is_contiguous() and v_t.is_cuda and w_t.is_cuda
        if v_t.dim() == 2:
            assert v_t.shape[0] == K and v_t.shape[1] in (1, B), tuple(v_t.shape)
            ld_tk, ld_tb = v_t.shape[1], (1 if v_t.shape[1] == B and B > 1 else 0)
        else:
            assert v_t.dim() == 1 and v_t.shape[0] in (1, B), tuple(v_t.shape)
            ld_tk, ld_tb = 0, (1 if v_t.shape[0] == B and B > 1 else 0)
        for t, shp, dt in (("u", (K, B, 6), torch.float64), ("x", (K, B, 8), torch.float64),
                           ("f", (K, B), torch.float64), ("fov", (K, B), torch.float64),
                           ("status", (K, B), torch.int32), ("iters", (K, B), torch.int32)):
            if hist.get(t) is not None:
                assert tuple(hist[t].shape) == shp and hist[t].dtype == dt and hist[t].is_contiguous(), t

        def op(k):
            t = hist.get(k)
            return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)

        ps_ld = 0
        if p_step is not None:
            assert p_step.dtype == torch.float64 and p_step.is_cuda and p_step.is_contiguous()
            assert tuple(p_step.shape) == (K, self.np), (tuple(p_step.shape), (K, self.np))
            ps_ld = self.np
        if order is not None:
            assert order.dtype == torch.int32 and order.is_cuda and order.is_contiguous()
            assert tuple(order.shape) == (B,), tuple(order.shape)
            # a dispatch order must be a permutation: a duplicate would run one scenario
            # on two waves at once (the completion check would still flag the missing one).
            # Checked on the synchronous path only: the check reads the device tensor back,
            # and check=False promises no host synchronisation (the device completion guard
            # reports a scenario a bad order leaves unrun)
            if check and _validate_order and not torch.equal(torch.sort(order).values,
                                                   torch.arange(B, dtype=torch.int32, device=order.device)):
                raise ValueError("order must be a permutation of range(B)")
        if stream is None:
            stream = torch.cuda.current_stream()
        _lib.check(L.nmpc_closed_loop_dev(self._h, B, K, *ins, C.c_void_p(p.data_ptr()), self.np,
                                          C.c_void_p(w.data_ptr()), C.c_void_p(v_t.data_ptr()),
                                          C.c_void_p(w_t.data_ptr()), ld_tk, ld_tb,
                                          C.c_void_p(p_step.data_ptr() if p_step is not None else 0), ps_ld,
                                          op("u"), op("x"),
                                          op("f"), op("fov"), op("status"), op("iters"),
                                          C.c_void_p(order.data_ptr() if order is not None else 0),
                                          C.c_void_p(stream.cuda_stream)))
        if check:
            self.check_closed_loop(B, K)

    def reserve_equality(self, B: int):
        """Allocate the equality class's device workspace for B scenarios (nmpc_reserve_eq):
        the device entry points (solve_device, closed_loop_device) never allocate it
        themselves, so that they never synchronise the host.  The host-array call
        (``solver(...)``) allocates it on demand."""
        _lib.check(_lib.lib().nmpc_reserve_eq(self._h, int(B)))

    def set_trace(self, enable: bool):
        _lib.check(_lib.lib().nmpc_set_trace(self._h, int(enable)))

    def read_trace(self, B: int) -> np.ndarray:
        buf = np.zeros((B, self.max_iter + 3, _lib.TRACE_FIELDS))
        _lib.check(_lib.lib().nmpc_read_trace(self._h, B, _dptr(buf)))
        return buf

    def closed_loop_info(self):
        """Scheduling of the last closed_loop_device launch (nmpc_closed_loop_info;
        synchronises the stream that launch was enqueued on before reading its flags)."""
        pol, res, err, wav, done = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        _lib.check(_lib.lib().nmpc_closed_loop_info(self._h, C.byref(pol), C.byref(res), C.byref(err),
                                                    C.byref(wav), C.byref(done)))
        return {"policy": ("step_queues" if pol.value == 1 else "per_scenario"), "resident_waves": res.value,
                "launched_waves": wav.value, "scheduler_error": err.value, "steps_done": done.value}

    def check_closed_loop(self, B: int, K: int):
        """Raise if the last closed-loop launch did not run every (scenario, step)."""
        info = self.closed_loop_info()
        if info["scheduler_error"] & 4:
            raise _lib.NmpcError("closed loop not run: the batch has equality rows (lbg == ubg) and the "
                                 "equality workspace is not reserved (Solver.reserve_equality(B)); the steps "
                                 f"carry status {_lib.EQ_UNRESERVED}")
        if info["scheduler_error"] != 0 or info["steps_done"] != B * K:
            raise _lib.NmpcError(f"closed loop incomplete: {info['steps_done']} of {B * K} steps run, "
                                 f"scheduler_error={info['scheduler_error']} (unrun steps carry status "
                                 f"{NOT_RUN} in the history)")
        return info

    def closed_loop_times(self, B: int, K: int):
        """Diagnostics (NMPC_STEP_TIMES set before the launch): (K, B, 3) uint64 --
        start / end s_memrealtime stamps (100 MHz) of every step and the running wave."""
        out = np.zeros((K, B, 3), dtype=np.uint64)
        _lib.check(_lib.lib().nmpc_closed_loop_times(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64)), out.size))
        return out

    def kernel_info(self):
        lds, tps = C.c_int32(), C.c_int32()
        _lib.check(_lib.lib().nmpc_kernel_info(self._h, C.byref(lds), C.byref(tps)))
        return {"lds_bytes": lds.value, "threads_per_scenario": tps.value}

    def memory_info(self):
        """Device workspace the handle holds: the problem class's, and the equality class's
        (allocated only once a batch with equality rows was solved); per-scenario sizes."""
        v = [C.c_int64() for _ in range(4)]
        _lib.check(_lib.lib().nmpc_memory_info(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("ws_bytes", "ws_eq_bytes", "ws_per_scenario", "ws_eq_per_scenario"), (x.value for x in v)))

    def stats(self) -> dict:
        return dict(self._stats)


def nlpsol(name: str, plugin: str, spec: ProblemSpec, opts: dict | None = None) -> Solver:
    """``ca.nlpsol(name, 'ipopt', nlp_prob, opts)`` for the NMPC_TT problem family."""
    if plugin != "ipopt":
        raise ValueError(f"only the 'ipopt' plugin is provided (got {plugin!r})")
    return Solver(name, spec, opts)
