// nmpc_solve_policy.hip -- the feedback policy along a plan in one launch
// (nmpc_solve_policy_batch / nmpc_solve_policy_batch_dev, include/nmpc_amd.h): for each of B
// scenarios at a solve's (x*, lam_g*, lam_x*), the neighbouring-extremal policy
//   u_k(x, p') ~ u*_k + K_k (x - X*_k) + sum_d kff_k^(d) c_d,   p' - p = sum_d c_d dp_d
// of the barrier-weighted LQ problem the fused sensitivity kernels solve: the time-varying gains
// K_k = -R~_k^-1 S~_k of the Riccati recursion at the delta ladder's delta, the
// stage matrices A_k, B_k of x_{k+1} = x_k + T f(x_k, u_k), the state trajectory X* and, per
// direction dp_d of the parameters, the feedforward
//   kff_k = k_k - K_k xi_k,   xi = (dX/dp) dp_d,
// with k_k of Solver::resolve on nmpc_solve_tangent_kernel's right-hand side, so that
// dx_k = K_k dX_k + kff_k for the dx, dX of nmpc_solve_tangent_kernel, every k.
//
// One difference from every sibling: stage 0's cross term S_0 = d2_xu (lam_1^T T f)^T, the two
// entries s03, s04 that nmpc_solve_tangent_kernel holds in registers, enters stage 0's summary
// before Solver::riccati (Q_0 stays 0).  K_0 multiplies dX~_0 = 0 in every solve, so no solve
// changes (k_0 = -R~_0^-1 r~_0 and the pivots do not read S_0); it makes the stored K_0 the
// stage-0 gain.
//
// Part of the evaluation kernel's translation unit (nmpc_eval.hip includes this file after
// nmpc_solve_tangent.hip): the solver's own text throughout; the LDS carve-up, the workspace
// slices, the steps up to the factorisation and each direction's right-hand side are
// nmpc_point.hip's, shared with nmpc_solve_adjoint.hip and nmpc_solve_tangent.hip.
//
// Execution model: the siblings'.  One wavefront per scenario, fp64, stage k on lane k, rows
// and variables strided over the lanes, control flow wave-uniform.
// Once per wavefront:
//   1. load_params, load_controls, point_rollout, point_weights (info = -11 and NaN outputs), point_derivs,
//      point_curvature, point_ladder with stage 0's cross term (info = 1 and NaN outputs);
//   2. lane k writes K_k (compacted to nu x nx, a fixed control's row 0.0), A_k, B_k and X*_k;
//      with directions and kff wanted, point_unit_grads.
// Per direction (the factorisation is shared):
//   3. point_direction_rhs and Solver::resolve;
//   4. kff = k - K xi, variables strided over the lanes, written through ext_u (a fixed
//      control's entry 0.0).
// Solver::forward, dlam_g and dX are not formed.
// (included by nmpc_eval.hip)

namespace {

__global__ __launch_bounds__(WAVE) void nmpc_solve_policy_kernel(const Params* __restrict__ prm, int B, SpolIO io) {
  __shared__ __attribute__((aligned(16))) double smem[T_TOTAL];
  const int b = blockIdx.x;
  if (b >= B) return;
  Solver<CapEv> S{};
  LDS double* sm = (LDS double*)smem;
  const PointRefs R = point_bind(S, prm, sm, io.pt, b);
  GLB double* xw = R.xw;
  const int N = S.N, nw = S.nw, nwE = S.nwE, nuE = S.nuE;
  const int npE = prm->npE, nxE = prm->nxE, nXE = nxE * (N + 1);
  const double T = S.T;
  const int lane = S.lanef(), k = lane;
  const double* db = io.dp ? io.dp + (long long)b * io.ld_dp : nullptr;
  const int nd = io.dp ? io.nd : 0;

  // every output of the scenario NaN (wave-uniform callers), its verdict and delta out
  auto finish_nan = [&](int verdict, double delta) {
    const long long nK = (long long)nuE * nxE * N, nA = (long long)nxE * nxE * N, nB = nK, nf = (long long)nd * nwE;
    nan_fill(io.K ? io.K + (long long)b * nK : nullptr, nK, lane);
    nan_fill(io.kff ? io.kff + (long long)b * nf : nullptr, nf, lane);
    nan_fill(io.A ? io.A + (long long)b * nA : nullptr, nA, lane);
    nan_fill(io.Bm ? io.Bm + (long long)b * nB : nullptr, nB, lane);
    nan_fill(io.X ? io.X + (long long)b * nXE : nullptr, nXE, lane);
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
  if (const int verdict = point_ladder(S, prm, R, k, cv.s03, cv.s04, delta)) {  // (stage 0's cross term too)
    finish_nan(verdict, delta);
    return;
  }
  sync();
  point_verdict(S, io.pt, lane, 0, delta);

  // ---------------- lane k: its stage's K_k (nu x nx of the stored 6 x 8, column-major), A_k,
  // B_k (column-major) and X*_k
  if (k < N) {
    const int fmk = S.fixm[k];
    if (io.K) {
      double* o = io.K + ((long long)b * N + k) * nuE * nxE;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          if (r < nuE && c < nxE) o[c * nuE + r] = ((fmk >> r) & 1) ? 0.0 : S.K[k * 48 + r * 8 + c];
        }
      }
    }
    if (io.A || io.Bm) {
      double e03, e04, e13, e14, e23, b00, b10, b20;
      S.stage_AB(k, e03, e04, e13, e14, e23, b00, b10, b20);
      if (io.A) {
        double* o = io.A + ((long long)b * N + k) * nxE * nxE;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            double v = r == c ? 1.0 : 0.0;
            if (r == 0 && c == 3) v = e03;
            if (r == 0 && c == 4) v = e04;
            if (r == 1 && c == 3) v = e13;
            if (r == 1 && c == 4) v = e14;
            if (r == 2 && c == 3) v = e23;
            if (r < nxE && c < nxE) o[c * nxE + r] = v;
          }
        }
      }
      if (io.Bm) {
        double* o = io.Bm + ((long long)b * N + k) * nxE * nuE;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            double v = 0.0;
            if (c == 0 && r == 0) v = b00;
            if (c == 0 && r == 1) v = b10;
            if (c == 0 && r == 2) v = b20;
            if (c >= 1 && r == 2 + c) v = T;
            if (r < nxE && c < nuE) o[c * nxE + r] = v;
          }
        }
      }
    }
  }
  if (io.X && k <= N) {
    double* o = io.X + (long long)b * nXE + k * nxE;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (c < nxE) o[c] = S.X[k * 8 + c];
    }
  }
  if (nd <= 0 || !io.kff) return;  // wave-uniform

  point_unit_grads(S, prm, R, lane);
  int pe;
  const bool reads = point_reads(S, prm, lane, pe);
  sync();

  // ---------------- directions
  for (int d = 0; d < nd; ++d) {
    point_direction_rhs(S, prm, R, lane, cv, db + (long long)d * npE, reads, pe);
    // the solve's backward half: k_k
    S.resolve(R.rv);
    // kff = k - K xi (xi_k as lane k stored it in point_direction_rhs)
    {
      double* o = io.kff + ((long long)b * nd + d) * nwE;
      for (int i = lane; i < nw; i += WAVE) {
        const int e = ext_u(prm, i);
        if (e < 0) continue;
        const int kk = i / 6, r = i - 6 * kk;
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < 8; ++c) acc += S.K[kk * 48 + r * 8 + c] * xw[kk * 8 + c];
        o[e] = S.fixed(i) ? 0.0 : S.kf[i] - acc;
      }
    }
    sync();
  }
}

}  // namespace

int nmpc_solve_policy_launch(const Params* dprm, int B, const SpolIO& io, void* stream) {
  hipLaunchKernelGGL(nmpc_solve_policy_kernel, dim3(B), dim3(WAVE), 0, (hipStream_t)stream, dprm, B, io);
  return (int)hipGetLastError();
}
