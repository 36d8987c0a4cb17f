// nmpc_solve_tangent.hip -- the forward-mode sensitivity of a SOLUTION in one launch
// (nmpc_solve_tangent_batch / nmpc_solve_tangent_batch_dev, include/nmpc_amd.h): for each of B
// scenarios at a solve's (x*, lam_g*, lam_x*) and each of nd directions dp of the parameters,
// with the barrier weights Sigma_x, Sigma_s of the point and
//   M = W + diag(Sigma_x) + delta I + J^T diag(Sigma_s + delta) J,
//   hp = (d_p grad_w L) dp,   jp = (dg/dp) dp,   dXp = (dX/dp) dp,
//   M dx = -hp - J^T Sigma_s jp,   dlam_g = Sigma_s (J dx + jp),   dX = (dX/dw) dx + dXp
// What Solver.sensitivity(tangent="exact") composes on the host from a launch of
// nmpc_pproducts.hip and launches of nmpc_kkt.hip, the weights in NumPy and the delta ladder as
// a Python loop, on the device -- and the state trajectory's tangent dX*, which no host route
// returns.  The forward-mode twin of nmpc_solve_adjoint.hip.
//
// Part of the evaluation kernel's translation unit (nmpc_eval.hip includes this file after
// nmpc_solve_adjoint.hip), so everything is the text the solver compiles; the LDS carve-up, the
// workspace slices, the steps up to the factorisation and each direction's right-hand side are
// nmpc_point.hip's, shared with nmpc_solve_adjoint.hip and nmpc_solve_policy.hip.
//
// Execution model: the siblings'.  One wavefront per scenario, fp64, stage k on lane k, rows
// and variables strided over the lanes, control flow wave-uniform.
// Once per wavefront:
//   1. to 4. load_params, load_controls, point_rollout, point_weights (info = -11 and NaN outputs),
//      point_derivs, point_curvature (what every direction's h_k needs, in registers),
//      point_ladder (info = 1 and NaN outputs), point_unit_grads.
// Per direction (the factorisation is shared):
//   5. to 10. point_direction_rhs: xi = (dX/dp) dp, h_k, jp, the reverse sweep, r_k and q_k;
//  11. Solver::resolve, Solver::forward: dx and (dX/dw) dx;
//  12. dlam_g = sigma_s (J dx + jp): the sum first, then the weight; stage 0's J dx is 0.0;
//  13. dX = (dX/dw) dx + xi, lane k its stage's.
// Every per-direction buffer is rewritten by each direction, so the directions are independent.
// (included by nmpc_eval.hip)

namespace {

__global__ __launch_bounds__(WAVE) void nmpc_solve_tangent_kernel(const Params* __restrict__ prm, int B, StanIO io) {
  __shared__ __attribute__((aligned(16))) double smem[T_TOTAL];
  const int b = blockIdx.x;
  if (b >= B) return;
  Solver<CapEv> S{};
  LDS double* sm = (LDS double*)smem;
  const PointRefs R = point_bind(S, prm, sm, io.pt, b);
  GLB double *dU = R.dU, *sg = R.sg, *jpv = R.yv, *xw = R.xw;
  LDS double* dX = sm + B_INC;   // (dX/dw) dx, from Solver::forward
  const int N = S.N, m = S.m, nw = S.nw, ng = S.ng, nwE = S.nwE;
  const int npE = prm->npE, nxE = prm->nxE, nXE = nxE * (N + 1);
  const int lane = S.lanef(), k = lane;
  const double* db = io.dp + (long long)b * io.ld_dp;

  // every output of the scenario NaN (wave-uniform callers), its verdict and delta out
  auto finish_nan = [&](int verdict, double delta) {
    const long long nd = io.nd;
    nan_fill(io.dx ? io.dx + (long long)b * nd * nwE : nullptr, nd * nwE, lane);
    nan_fill(io.dlam_g ? io.dlam_g + (long long)b * nd * ng : nullptr, nd * ng, lane);
    nan_fill(io.dX ? io.dX + (long long)b * nd * nXE : nullptr, nd * nXE, lane);
    point_verdict(S, io.pt, lane, verdict, delta);
  };

  load_params(S, prm, lane, io.pt.p + (long long)b * io.pt.ld_p);
  load_controls(S, prm, lane, R.xb, true);
  sync();
  point_rollout(S, lane);
  if (point_weights(S, prm, R, k)) {
    finish_nan(-11, 0.0);
    return;
  }
  point_derivs(S, R);
  const PointCurv cv = point_curvature(S, R, k);
  double delta;
  if (const int verdict = point_ladder(S, prm, R, k, 0.0, 0.0, delta)) {
    finish_nan(verdict, delta);
    return;
  }
  sync();
  point_verdict(S, io.pt, lane, 0, delta);
  point_unit_grads(S, prm, R, lane);
  int pe;
  const bool reads = point_reads(S, prm, lane, pe);
  sync();

  // ---------------- directions
  for (int d = 0; d < io.nd; ++d) {
    point_direction_rhs(S, prm, R, lane, cv, db + (long long)d * npE, reads, pe);
    // 11. the solves: dx and its state step
    S.resolve(R.rv);
    S.forward(dU, dX);
    if (io.dx) {
      double* o = io.dx + ((long long)b * io.nd + d) * nwE;
      for (int i = lane; i < nw; i += WAVE) {
        const int e = ext_u(prm, i);
        if (e < 0) continue;
        o[e] = S.fixed(i) ? 0.0 : dU[i];
      }
    }
    // 12. dlam_g = sigma_s (J dx + jp) (stage 0's rows: J is zero there)
    if (io.dlam_g) {
      double* o = io.dlam_g + ((long long)b * io.nd + d) * ng;
      for (int r = lane; r < ng; r += WAVE) {
        const double jq = r < m ? 0.0 : S.row_jd(r, dX);
        o[r] = sg[r] * (jq + jpv[r]);
      }
    }
    // 13. dX = (dX/dw) dx + xi
    if (io.dX && k <= N) {
      double* o = io.dX + ((long long)b * io.nd + d) * nXE;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        if (c < nxE) o[k * nxE + c] = dX[k * 8 + c] + xw[k * 8 + c];
      }
    }
    sync();
  }
}

}  // namespace

int nmpc_solve_tangent_launch(const Params* dprm, int B, const StanIO& io, void* stream) {
  hipLaunchKernelGGL(nmpc_solve_tangent_kernel, dim3(B), dim3(WAVE), 0, (hipStream_t)stream, dprm, B, io);
  return (int)hipGetLastError();
}
