// nmpc_kkt.hip -- batched solves with the condensed KKT matrix at GIVEN points
// (nmpc_kkt_solve_batch / nmpc_kkt_solve_batch_dev, include/nmpc_amd.h): for each of B
// scenarios and each of nr right-hand sides
//   M dw = r_w + J^T r_g,   M = W + diag(sigma_x) + delta I + J^T diag(sigma_s + delta) J,
//   W = obj_factor grad^2 f + sum_i lam_g_i grad^2 g_i,
// IPOPT's primal-dual system with the slacks and bound multipliers eliminated,
// with the state step dX = (dX/dw) dw and the row step J dw.  The solver's own Riccati
// factorisation, its solves and its inertia verdict, reachable without an interior-point
// iteration around them.
//
// Part of the evaluation kernel's translation unit: nmpc_eval.hip includes this file after
// nmpc_products.hip, so the solver's source is seen with no class selected and the linear
// algebra here is the text the solver compiles -- Solver::riccati (factorisation, inertia),
// Solver::resolve (the gradient-only backward pass with the stored factors), Solver::forward,
// Solver::row_jd -- on the derivatives of Solver::derivs<true> and Solver::adjoint.
//
// Execution model: the solver's.  One wavefront per scenario, fp64, control flow wave-uniform.
// Once per wavefront:
//   1. scenario data, rollout and stage costs (load_params, load_controls, point_rollout of
//      nmpc_eval_shared.hip: the stage costs fill the transcendental cache that
//      derivs<true, true> reads);
//   2. the weights: sigma_x into the kernel's 6-per-stage layout (+inf: the variable is fixed,
//      Solver::fixm, as make_parameter's), sigma_s and delta checked; an invalid weight ends
//      the scenario with info = -11 and NaN outputs;
//   3. derivs<true, true>: gl, Hl; adjoint(obj_factor, lam_g): lam_{k+1};
//   4. lane k: the stage summary Q_k = obj_factor Hl_k + G_k^T (sigma_s + delta) G_k
//      + sum_o lam_{k,o} Hg_o + the dynamics terms of lam_{k+1}^T T f, and S_k's two entries
//      -- the expressions of Solver::assemble's Newton mode with D = sigma_s + delta, for
//      k >= 1 (stage 0 is constant in w: Q_0 = 0, none of its terms is formed);
//   5. Solver::riccati once, with zero linear terms: K_k, R~_k; a pivot that is not positive
//      ends the scenario with info = 1 and NaN outputs.
// Per right-hand side:
//   6. r_k = -r_w (controls), q_k = -G_k^T r_g (k >= 1): the solver's recursion solves
//      M dw = -(r + Z^T q);
//   7. Solver::resolve, Solver::forward: dw, dX;
//   8. J dw: row (k, i) = G_{k,i} dX_k (Solver::row_jd).
// Every per-right-hand-side buffer is rewritten by each one, so the columns are independent.
// (included by nmpc_eval.hip)

namespace {

static_assert(fits_every_class(kKktWs),
              "a solver class's workspace is smaller than one wavefront's of the KKT kernel");
static_assert(std::is_same<CapEv::RT, double>::value && !CapEv::deep && !CapEv::eq,
              "the KKT kernel runs the fp64 factorisation of the global-row class");

// LDS carve-up (doubles): the unit's head (its prefix-sum scratch also holds the sweeps' P / p
// buffers), then
constexpr int K_DX = B_END;                   // the right-hand side's state step
constexpr int K_QS = K_DX + 8 * NS;           // q_k (8), S_k[0][3], S_k[0][4] per stage
constexpr int K_SW = K_QS + 10 * NS;          // S~ (48), R~ (22), r~ (8) of the current stage
constexpr int K_FIX = K_SW + 48 + 22 + 8;     // fixed-control masks, one int per stage
constexpr int K_TOTAL = K_FIX + NS / 2 + 2;
static_assert(8 * NS >= 144, "the sweeps' P / p buffers live in the prefix-sum scratch");
static_assert(K_TOTAL * 8 <= 32 * 1024, "KKT kernel LDS");

__global__ __launch_bounds__(WAVE) void nmpc_kkt_kernel(const Params* __restrict__ prm, int B, KktIO io) {
  __shared__ __attribute__((aligned(16))) double smem[K_TOTAL];
  const int b = blockIdx.x;
  if (b >= B) return;
  Solver<CapEv> S{};
  LDS double* sm = (LDS double*)smem;
  GLB double* gw = (GLB double*)(io.ws + (long long)b * kKktWs);
  bind_solver(S, prm, sm, gw, b, kKktU, kKktGl, kKktHl, kKktTc, kKktDc);
  S.Qs = gw + kKktQs; S.K = gw + kKktK; S.Rk = gw + kKktRk; S.kf = gw + kKktKf;
  GLB double* Rd = gw + kKktRd;  // sigma_x, the kernel's layout
  GLB double* rv = gw + kKktRv;  // the right-hand side's control terms
  GLB double* dU = gw + kKktDu;  // its step
  S.qs = sm + K_QS;
  S.Pa = S.inc; S.Pb = S.inc + 64; S.pva = S.inc + 128; S.pvb = S.inc + 136;
  S.St = sm + K_SW; S.Rc = S.St + 48; S.Rv = S.Rc + 22;
  S.fixm = (LDS int*)(sm + K_FIX);
  LDS double* dX = sm + K_DX;
  const int N = S.N, m = S.m, nw = S.nw, ng = S.ng, nwE = S.nwE, nuE = S.nuE;
  const int nXE = prm->nxE * (N + 1);
  const int lane = S.lanef();
  const double* yb = io.lam_g ? io.lam_g + (long long)b * io.ld_lam_g : nullptr;
  const double* xb = io.x + (long long)b * io.ld_x;
  const double* sxb = io.sigma_x ? io.sigma_x + (long long)b * io.ld_sigma_x : nullptr;
  const double* ssb = io.sigma_s ? io.sigma_s + (long long)b * io.ld_sigma_s : nullptr;
  const double* rwb = io.r_w ? io.r_w + (long long)b * io.ld_r_w : nullptr;
  const double* rgb = io.r_g ? io.r_g + (long long)b * io.ld_r_g : nullptr;
  const double delta = io.delta ? io.delta[(long long)b * io.ld_delta] : 0.0;
  S.delta = delta;

  // every output of the scenario NaN (wave-uniform callers), its verdict to info_out
  auto finish_nan = [&](int verdict) {
    const long long nr = io.nr;
    if (io.dw)
      for (long long i = lane; i < nr * nwE; i += WAVE) io.dw[(long long)b * nr * nwE + i] = NAN;
    if (io.dX)
      for (long long i = lane; i < nr * nXE; i += WAVE) io.dX[(long long)b * nr * nXE + i] = NAN;
    if (io.jdw)
      for (long long i = lane; i < nr * ng; i += WAVE) io.jdw[(long long)b * nr * ng + i] = NAN;
    if (io.info && lane == 0) io.info[b] = verdict;
  };

  // ---------------- scenario data
  load_params(S, prm, lane, io.p + (long long)b * io.ld_p);
  load_controls(S, prm, lane, xb, true);

  // ---------------- the weights: sigma_x (lane k: its stage's controls, +inf = fixed), sigma_s
  bool bad = !(delta >= 0.0) || delta == INFINITY;
  int fmk = 0;
  if (lane < N) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const double v = (sxb && c < nuE) ? sxb[lane * nuE + c] : 0.0;
      const bool fx = v == INFINITY;
      bad |= !(v >= 0.0);
      fmk |= fx ? (1 << c) : 0;
      Rd[lane * 6 + c] = fx ? 0.0 : v;
      rv[lane * 6 + c] = 0.0;
    }
  }
  if (lane <= N) S.fixm[lane] = fmk;
  if (ssb)
    for (int r = m + lane; r < ng; r += WAVE) {  // stage 0's rows have no effect: never read
      const double v = ssb[r];
      bad |= !(v >= 0.0) || v == INFINITY;
    }
  S.nfix = wany(fmk != 0) ? 1 : 0;
  if (wany(bad)) {
    finish_nan(-11);
    return;
  }
  sync();

  // ---------------- rollout, stage costs (their transcendentals), derivatives, multipliers
  point_rollout(S, lane);
  S.derivs<true, true>(S.X, S.U, S.tc);
  if (yb) S.adjoint(io.obj_factor, yb);
  else S.adjoint(io.obj_factor, (const double*)nullptr);

  // ---------------- lane k: the stage summary (Solver::assemble's Newton mode, D = sigma_s + delta)
  const int k = lane;
  point_summary(S, k, io.obj_factor, ssb, yb, delta, 0.0, 0.0);
  sync();

  // ---------------- factorisation and inertia (zero linear terms)
  if (!S.riccati(Rd, rv)) {
    finish_nan(1);
    return;
  }
  sync();
  if (io.info && lane == 0) io.info[b] = 0;

  // ---------------- right-hand sides
  for (int d = 0; d < io.nr; ++d) {
    // 6. r_k = -r_w, q_k = -G_k^T r_g
    for (int i = lane; i < nw; i += WAVE) {
      const int e = ext_u(prm, i);
      rv[i] = (rwb && e >= 0) ? -rwb[(long long)d * nwE + e] : 0.0;
    }
    if (k >= 1 && k <= N) {
      const double* rg = rgb ? rgb + (long long)d * ng : nullptr;
      point_stage_q(S, k, rg != nullptr, [&](int i) { return -rg[k * m + i]; });
    }
    sync();
    // 7. the solves
    S.resolve(rv);
    S.forward(dU, dX);
    // 8. outputs
    if (io.dw) {
      double* o = io.dw + ((long long)b * io.nr + d) * nwE;
      for (int i = lane; i < nw; i += WAVE) {
        const int e = ext_u(prm, i);
        if (e < 0) continue;
        o[e] = S.fixed(i) ? 0.0 : dU[i];
      }
    }
    if (io.jdw) put_rows_jd(S, lane, dX, io.jdw + ((long long)b * io.nr + d) * ng);
    if (io.dX) put_trajectory(prm, lane, dX, io.dX + ((long long)b * io.nr + d) * nXE);
    sync();
  }
}

}  // namespace

int nmpc_kkt_launch(const Params* dprm, int B, const KktIO& io, void* stream) {
  hipLaunchKernelGGL(nmpc_kkt_kernel, dim3(B), dim3(WAVE), 0, (hipStream_t)stream, dprm, B, io);
  return (int)hipGetLastError();
}
