// nmpc_solve_adjoint.hip -- the reverse-mode sensitivity of a SOLUTION in one launch
// (nmpc_solve_adjoint_batch / nmpc_solve_adjoint_batch_dev, include/nmpc_amd.h): for each of B
// scenarios at a solve's (x*, lam_g*, lam_x*) and each of na seeds (x_bar on x*, lam_g_bar on
// lam_g*, X_bar on X*), with the barrier weights Sigma_x, Sigma_s of the point and
//   M = W + diag(Sigma_x) + delta I + J^T diag(Sigma_s + delta) J,
//   q = M^-1 (x_bar + (dX/dw)^T X_bar + J^T Sigma_s lam_g_bar),
//   pbar = -(d_p grad_w L)^T q + (dg/dp)^T Sigma_s (lam_g_bar - J q) + (dX/dp)^T X_bar
// so that <pbar, dp> = <x_bar, dx*> + <lam_g_bar, dlam_g*> + <X_bar, dX*> for every dp.  What
// Solver.sensitivity_adjoint composes on the host from three launches of nmpc_adjoint.hip and
// nmpc_kkt.hip, the weights in NumPy and the delta ladder as a Python loop, on the device.
//
// Part of the evaluation kernel's translation unit (nmpc_eval.hip includes this file last), so
// everything is the text the solver compiles: Solver::rollout, stage_cost, row_value,
// derivs<true, true>, adjoint, riccati, resolve, forward, row_jd, stage_AB, grad_u, and the
// curvature expressions of nmpc_kkt.hip / nmpc_adjoint.hip.
//
// Execution model: the siblings'.  One wavefront per scenario, fp64, stage k on lane k, rows
// and variables strided over the lanes, control flow wave-uniform.
// Once per wavefront:
//   1. scenario data, rollout and stage costs as nmpc_kkt_kernel; where a cost weight comes from
//      p, the unit-weight stage-cost gradients as nmpc_adjoint_kernel (formed after step 4, into
//      the stage summaries' slice, which is dead by then); derivs<true, true> and
//      adjoint(1, lam_g): gl, Hl, lam_{k+1} (the objective factor is 1);
//   2. the barrier weights, Solver.barrier_weights' operations in their order:
//        sl = max(v - lo, brf max(1, |lo|)), su = max(hi - v, brf max(1, |hi|)),
//        sigma = max(-lam, 0) / sl + max(lam, 0) / su
//      (max as numpy.maximum: a NaN stays); lane k its stage's controls (lbx == ubx: +inf, the
//      variable leaves the system, Solver::fixm) and its stage's rows (v = the given g, else
//      the kernel's own row value); an equality row, lbx > ubx or a weight that is not a
//      finite non-negative number ends the scenario with info = -11 and NaN outputs;
//   3. lane k keeps the second-order data every seed's pullback needs: the summed obstacle
//      curvature and the dynamics terms d33, d34, d44, s03, s04 of lam_{k+1}^T T f (stage 0's
//      included: its Hxu_0 z_0 reaches the x0 block of pbar);
//   4. the delta ladder: delta = 0, the stage summaries Q_k with D = sigma_s + delta
//      (nmpc_kkt_kernel's text), Solver::riccati; on a failed inertia verdict the next rung
//      (first_hessian_perturbation, then x perturb_inc_fact_first, then x perturb_inc_fact: the
//      host ladder's multiplications) while it is <= max_hessian_perturbation; beyond it
//      info = 1 and NaN outputs.
// Per seed (the factorisation is shared):
//   5. r_w = x_bar + (dX/dw)^T X_bar -- with X_bar, one reverse sweep (Solver::adjoint on the
//      stage sources X_bar_k, grad_u) -- and q_k = -G_k^T (sigma_s lam_g_bar);
//   6. Solver::resolve, Solver::forward: q, and its state step dX = (dX/dw) q; J q by row_jd;
//   7. y = sigma_s (lam_g_bar - J q) into the workspace, z = -q;
//   8. the pullback of (y, z, X_bar) to p as nmpc_adjoint_kernel's steps 6 to 9, with the
//      tangent of z taken from the forward sweep (xi = -dX: no second prefix-sum tangent) and an
//      obstacle's own curvature lam_{k,o} Hg_o recomputed where its centre comes from p.
// Every per-seed buffer is rewritten by each seed, so the seeds are independent.
// (included by nmpc_eval.hip)

namespace {

static_assert(CapA::L.wstotal >= kSadjWs && CapB::L.wstotal >= kSadjWs && CapC::L.wstotal >= kSadjWs &&
                  CapD::L.wstotal >= kSadjWs && CapA32::L.wstotal >= kSadjWs && CapC32::L.wstotal >= kSadjWs &&
                  CapE::L.wstotal >= kSadjWs,
              "a solver class's workspace is smaller than one wavefront's of the fused sensitivity kernel");

// LDS carve-up (doubles): the KKT kernel's without a buffer of its own for the state step, which
// lives in the prefix-sum scratch: Solver::forward reads nothing there, every lane takes its
// stage's entries into registers before the pullback's sweep uses the scratch again, and the
// next seed's sweeps find it dead.  23.6 KB: six workgroups per CU's 160 KiB, where the KKT
// kernel's 27.7 KB allow five
constexpr int A_PP = 0;                       // p, internal layout (<= 64)
constexpr int A_OB = A_PP + 64;               // obstacle x (16), y (16)
constexpr int A_RV = A_OB + 2 * NMPC_MAX_OBS; // Solver::rvars; [30], [31] = cost weights
constexpr int A_ST = A_RV + 32;               // phase-timer slots (NMPC_STAMPS builds write them)
constexpr int A_X = A_ST + PH_COUNT;          // trajectory, 8 per stage
constexpr int A_TRIG = A_X + 8 * NS;
constexpr int A_INC = A_TRIG + 8 * NS;        // prefix / suffix sum scratch; the sweeps' P / p buffers; the
                                              // seed's state step (dX/dw) q between forward and pullback
constexpr int A_LAM = A_INC + 8 * NS;         // lam, then each seed's nu
constexpr int A_QS = A_LAM + 8 * NS;          // q_k (8), S_k[0][3], S_k[0][4] per stage
constexpr int A_SW = A_QS + 10 * NS;          // S~ (48), R~ (22), r~ (8) of the current stage
constexpr int A_FIX = A_SW + 48 + 22 + 8;     // fixed-control masks, one int per stage
constexpr int A_TOTAL = A_FIX + NS / 2 + 2;
static_assert(A_TOTAL * 8 <= 32 * 1024, "fused sensitivity kernel LDS");

// numpy.maximum: a NaN operand stays (fmax would drop it)
__device__ __forceinline__ double npmax(double a, double b) { return (a != a || b != b) ? NAN : (a > b ? a : b); }
// Solver.barrier_weights' weight of one value between its bounds
__device__ __forceinline__ double barrier_sigma(double v, double lam, double lo, double hi, double brf) {
  const double sl = npmax(v - lo, brf * npmax(1.0, fabs(lo)));
  const double su = npmax(hi - v, brf * npmax(1.0, fabs(hi)));
  return npmax(-lam, 0.0) / sl + npmax(lam, 0.0) / su;
}

__global__ __launch_bounds__(WAVE) void nmpc_solve_adjoint_kernel(const Params* __restrict__ prm, int B, SadjIO io) {
  __shared__ __attribute__((aligned(16))) double smem[A_TOTAL];
  const int b = blockIdx.x;
  if (b >= B) return;
  Solver<CapEv> S{};
  LDS double* sm = (LDS double*)smem;
  GLB double* gw = (GLB double*)(io.ws + (long long)b * kSadjWs);
  S.P = (const CST Params*)prm; S.sm = sm; S.lane_ = threadIdx.x; S.b = b;
  S.N = prm->N; S.m = prm->m; S.nobs = prm->nobs; S.nw = prm->nw; S.ng = prm->ng; S.T = prm->T;
  S.nb = prm->nb; S.nuE = prm->nuE; S.nwE = prm->nwE;
  S.U = gw + kKktU; S.gl = gw + kKktGl; S.Hl = gw + kKktHl; S.tc = gw + kKktTc; S.dc = gw + kKktDc;
  S.Qs = gw + kKktQs; S.K = gw + kKktK; S.Rk = gw + kKktRk; S.kf = gw + kKktKf;
  GLB double* Rd = gw + kKktRd;  // sigma_x, the kernel's layout
  GLB double* rv = gw + kKktRv;  // the seed's control terms
  GLB double* dU = gw + kKktDu;  // its q
  GLB double* sg = gw + kSadjSg; // sigma_s
  GLB double* yv = gw + kSadjY;  // the seed's y
  GLB double* uw = gw + kKktQs;  // after the ladder: unit-weight stage-cost gradients, 6 + 6 per stage
  S.pp = sm + A_PP; S.obx = sm + A_OB; S.oby = S.obx + NMPC_MAX_OBS; S.rvars = sm + A_RV; S.stamps = sm + A_ST;
  S.X = sm + A_X; S.trig = sm + A_TRIG; S.inc = sm + A_INC; S.lam = sm + A_LAM; S.qs = sm + A_QS;
  S.Pa = S.inc; S.Pb = S.inc + 64; S.pva = S.inc + 128; S.pvb = S.inc + 136;
  S.St = sm + A_SW; S.Rc = S.St + 48; S.Rv = S.Rc + 22;
  S.fixm = (LDS int*)(sm + A_FIX);
  LDS double* dX = sm + A_INC;
  const int N = S.N, m = S.m, nb = S.nb, nw = S.nw, ng = S.ng, nwE = S.nwE, nuE = S.nuE;
  const int np = prm->np, npE = prm->npE, nxE = prm->nxE, nXE = nxE * (N + 1);
  const int w1p = prm->w1p, w2p = prm->w2p;
  const double T = S.T;
  const int lane = S.lanef();
  const double* xb = io.x + (long long)b * io.ld_x;
  const double* yb = io.lam_g + (long long)b * io.ld_lam_g;
  const double* lxb = io.lam_x + (long long)b * io.ld_lam_x;
  const double* gb = io.g ? io.g + (long long)b * io.ld_g : nullptr;
  const double* lbxb = io.lbx + (long long)b * io.ld_lbx;
  const double* ubxb = io.ubx + (long long)b * io.ld_ubx;
  const double* lbgb = io.lbg + (long long)b * io.ld_lbg;
  const double* ubgb = io.ubg + (long long)b * io.ld_ubg;
  const double* xs = io.x_bar ? io.x_bar + (long long)b * io.ld_x_bar : nullptr;
  const double* ls = io.lam_g_bar ? io.lam_g_bar + (long long)b * io.ld_lam_g_bar : nullptr;
  const double* Xs = io.X_bar ? io.X_bar + (long long)b * io.ld_X_bar : nullptr;
  S.delta = 0.0;

  // every output of the scenario NaN (wave-uniform callers), its verdict and delta out
  auto finish_nan = [&](int verdict, double delta) {
    const long long na = io.na;
    if (io.pbar)
      for (long long i = lane; i < na * npE; i += WAVE) io.pbar[(long long)b * na * npE + i] = NAN;
    if (io.q)
      for (long long i = lane; i < na * nwE; i += WAVE) io.q[(long long)b * na * nwE + i] = NAN;
    if (io.jq)
      for (long long i = lane; i < na * ng; i += WAVE) io.jq[(long long)b * na * ng + i] = NAN;
    if (lane == 0) {
      if (io.info) io.info[b] = verdict;
      if (io.delta) io.delta[b] = delta;
    }
  };

  // ---------------- scenario data (as nmpc_kkt_kernel loads it)
  if (lane < PH_COUNT) S.stamps[lane] = 0.0;
  for (int i = lane; i < np; i += WAVE) {
    const int e = ext_p(prm, i);
    S.pp[i] = e >= 0 ? io.p[(long long)b * io.ld_p + e] : 0.0;
  }
  sync();
  if (lane < NMPC_MAX_OBS) {
    const bool on = lane < S.nobs;
    S.obx[lane] = on ? (prm->oxp[lane] >= 0 ? S.pp[prm->oxp[lane]] : prm->ox[lane]) : 0.0;
    S.oby[lane] = on ? (prm->oyp[lane] >= 0 ? S.pp[prm->oyp[lane]] : prm->oy[lane]) : 0.0;
  }
  if (lane == 0) {
    S.rvars[30] = w1p >= 0 ? S.pp[w1p] : prm->w1;
    S.rvars[31] = w2p >= 0 ? S.pp[w2p] : prm->w2;
  }
  for (int i = lane; i < nw; i += WAVE) {
    const int e = ext_u(prm, i);
    S.U[i] = e >= 0 ? xb[e] : 0.0;
  }
  for (int r = lane; r < ng; r += WAVE) S.dc[r] = 1.0;  // unscaled rows
  sync();

  // ---------------- rollout and stage costs (their transcendentals)
  S.rollout(S.U, S.X);
  if (lane < N) (void)S.stage_cost(S.X + lane * 8, S.tc + lane * 12);
  sync();

  const int k = lane;
  const bool stage = k >= 1 && k <= N;  // the stages whose state depends on w
  const int sv[6] = {0, 1, 2, 5, 6, 7};  // the states a stage cost reads

  // ---------------- the barrier weights: lane k its stage's controls and rows
  {
    const double brf = prm->o.bound_relax_factor;
    bool bad = false;
    int fmk = 0;
    if (k < N) {
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        double v = 0.0;
        if (c < nuE) {
          const int e = k * nuE + c;
          const double lo = lbxb[e], hi = ubxb[e];
          v = lo == hi ? INFINITY : barrier_sigma(xb[e], lxb[e], lo, hi, brf);
          bad |= lo > hi;
        }
        const bool fx = v == INFINITY;
        bad |= !(v >= 0.0);
        fmk |= fx ? (1 << c) : 0;
        Rd[k * 6 + c] = fx ? 0.0 : v;
        rv[k * 6 + c] = 0.0;
      }
    }
    if (k <= N) {
      S.fixm[k] = fmk;
      const LDS double* xk = S.X + k * 8;
      for (int i = 0; i < m; ++i) {
        const int r = k * m + i;
        const double lo = lbgb[r], hi = ubgb[r];
        const double v = barrier_sigma(gb ? gb[r] : S.row_value(xk, i), yb[r], lo, hi, brf);
        bad |= lo == hi || !(v >= 0.0) || v == INFINITY;
        sg[r] = v;
      }
    }
    S.nfix = wany(fmk != 0) ? 1 : 0;
    if (wany(bad)) {
      finish_nan(-11, 0.0);
      return;
    }
  }

  // ---------------- derivatives and multipliers at the scenario's own weights
  S.derivs<true, true>(S.X, S.U, S.tc);
  S.adjoint(1.0, yb);

  // second derivatives of lam_{k+1}^T T f(x_k, u_k), stage k < N on lane k (nmpc_kkt_kernel's
  // expressions): added to the three entries of d2_xx, and S_k's two entries
  auto dyn2 = [&](double& a33, double& a44, double& a34, double& b03, double& b04) {
    const LDS double* tg = S.trig + k * 8;
    const double ct = tg[0], stt = tg[1], cp = tg[2], sp = tg[3], v = tg[4];
    const LDS double* ln = S.lam + (k + 1) * 8;
    const double l0 = ln[0], l1 = ln[1], l2 = ln[2];
    a33 += T * (-l0 * v * cp * ct - l1 * v * sp * ct - l2 * v * stt);
    a44 += T * (-l0 * v * cp * ct - l1 * v * sp * ct);
    a34 += T * (l0 * v * sp * stt - l1 * v * cp * stt);
    b03 = T * (-l0 * cp * stt - l1 * sp * stt + l2 * ct);
    b04 = T * (-l0 * sp * ct + l1 * cp * ct);
  };

  // ---------------- lane k: the second-order data of every seed's pullback, in registers
  double q00 = 0.0, q01 = 0.0, q11 = 0.0;
  double d33 = 0.0, d34 = 0.0, d44 = 0.0, s03 = 0.0, s04 = 0.0;  // (stage 0's s03, s04 are not in qs)
  if (io.pbar) {
    if (stage) {  // lam_g-weighted obstacle curvature: nmpc_adjoint_kernel's, rows in order
      const LDS double* xk = S.X + k * 8;
      for (int o = 0; o < S.nobs; ++o) {
        const double C = yb[k * m + nb + o];
        const double ddx = xk[0] - S.obx[o], ddy = xk[1] - S.oby[o];
        const double idd = rsq(ddx * ddx + ddy * ddy);
        const double id3 = idd * idd * idd;
        q00 += C * (-ddy * ddy * id3); q01 += C * (ddx * ddy * id3); q11 += C * (-ddx * ddx * id3);
      }
    }
    if (k < N) dyn2(d33, d44, d34, s03, s04);
  }

  // ---------------- the delta ladder: stage summaries (nmpc_kkt_kernel's text) and factorisation
  double delta = 0.0;
  int verdict = 0;
  {
    const double first = prm->o.first_hessian_perturbation, inc_first = prm->o.perturb_inc_fact_first;
    const double inc = prm->o.perturb_inc_fact, dmax = prm->o.max_hessian_perturbation;
    while (true) {
      S.delta = delta;
      if (k <= N) {
        double Q[36];
#pragma unroll
        for (int t = 0; t < 36; ++t) Q[t] = 0.0;
        double r03 = 0.0, r04 = 0.0;
        if (k >= 1) {  // the stages whose state depends on w
          const LDS double* xk = S.X + k * 8;
          double Qxy0 = 0, Qxy1 = 0, Qxy2 = 0;
          double Qb[5] = {0, 0, 0, 0, 0};
          for (int i = 0; i < m; ++i) {
            const int r = k * m + i;
            const double w = sg[r] + delta;
            if (i < nb) {
              Qb[i] = w;
            } else {
              const double C = yb[r];
              const int o = i - nb;
              const double ddx = xk[0] - S.obx[o], ddy = xk[1] - S.oby[o];
              const double idd = rsq(ddx * ddx + ddy * ddy);
              const double gx = -(ddx * idd), gy = -(ddy * idd);
              const double id3 = idd * idd * idd;
              Qxy0 += w * gx * gx + C * (-ddy * ddy * id3);
              Qxy1 += w * gx * gy + C * (ddx * ddy * id3);
              Qxy2 += w * gy * gy + C * (-ddx * ddx * id3);
            }
          }
#pragma unroll
          for (int a = 0; a < 6; ++a) {
#pragma unroll
            for (int bq = a; bq < 6; ++bq) Q[S.pk8(sv[a], sv[bq])] += S.Hl[k * 21 + hp(a, bq)];
          }
          Q[S.pk8(0, 0)] += Qxy0; Q[S.pk8(0, 1)] += Qxy1; Q[S.pk8(1, 1)] += Qxy2;
          Q[S.pk8(2, 2)] += Qb[0]; Q[S.pk8(3, 3)] += Qb[1]; Q[S.pk8(5, 5)] += Qb[2];
          Q[S.pk8(6, 6)] += Qb[3]; Q[S.pk8(7, 7)] += Qb[4];
          if (k < N) dyn2(Q[S.pk8(3, 3)], Q[S.pk8(4, 4)], Q[S.pk8(3, 4)], r03, r04);
        }
#pragma unroll
        for (int t = 0; t < 36; ++t) S.Qs[k * 36 + t] = Q[t];
        LDS double* qo = S.qs + k * 10;
#pragma unroll
        for (int c = 0; c < 8; ++c) qo[c] = 0.0;
        qo[8] = r03;
        qo[9] = r04;
      }
      sync();
      if (S.riccati(Rd, rv)) break;  // zero linear terms
      sync();
      // the next rung, by the host ladder's multiplications
      const double nxt = delta == 0.0 ? first : (delta == first ? inc_first * delta : inc * delta);
      if (!(nxt <= dmax) || !(nxt > delta)) {  // (a ladder that does not climb ends here too)
        verdict = 1;
        break;
      }
      delta = nxt;
    }
  }
  if (verdict != 0) {
    finish_nan(verdict, delta);
    return;
  }
  sync();
  if (lane == 0) {
    if (io.info) io.info[b] = 0;
    if (io.delta) io.delta[b] = delta;
  }
  // ---------------- cost weights from p: unit-weight gradients, lane k stage k's, into the stage
  // summaries' slice (dead once the factorisation stands; the gradient slice is each seed's)
  if (io.pbar && (w1p >= 0 || w2p >= 0)) {
    const double w1s = S.rvars[30], w2s = S.rvars[31];
    sync();
    if (w1p >= 0) {
      if (lane == 0) { S.rvars[30] = 1.0; S.rvars[31] = 0.0; }
      sync();
      S.derivs<false, true>(S.X, S.U, S.tc);
      if (k < N) {
#pragma unroll
        for (int a = 0; a < 6; ++a) uw[k * 12 + a] = S.gl[k * 8 + sv[a]];
      }
    }
    if (w2p >= 0) {
      if (lane == 0) { S.rvars[30] = 0.0; S.rvars[31] = 1.0; }
      sync();
      S.derivs<false, true>(S.X, S.U, S.tc);
      if (k < N) {
#pragma unroll
        for (int a = 0; a < 6; ++a) uw[k * 12 + 6 + a] = S.gl[k * 8 + sv[a]];
      }
    }
    if (lane == 0) { S.rvars[30] = w1s; S.rvars[31] = w2s; }
    sync();
  }

  // the internal entry of p this lane forms, and its place in the caller's layout
  const int pe = lane < np ? ext_p(prm, lane) : -1;

  // ---------------- seeds
  for (int d = 0; d < io.na; ++d) {
    const double* xd = xs ? xs + (long long)d * nwE : nullptr;
    const double* ld = ls ? ls + (long long)d * ng : nullptr;
    const double* Xd = Xs ? Xs + (long long)d * nXE : nullptr;
    // 5. r_k = -(x_bar + (dX/dw)^T X_bar), q_k = -G_k^T (sigma_s lam_g_bar)
    if (Xd) {
      if (k <= N) {
        GLB double* h = S.gl + k * 8;
#pragma unroll
        for (int c = 0; c < 8; ++c) h[c] = c < nxE ? Xd[k * nxE + c] : 0.0;
      }
      sync();
      S.adjoint(1.0, (const double*)nullptr);
    }
    for (int i = lane; i < nw; i += WAVE) {
      const int e = ext_u(prm, i);
      double r = 0.0;
      if (e >= 0) {
        if (Xd) {
          const double g = S.grad_u(i);
          r = -(xd ? xd[e] + g : g);
        } else if (xd) {
          r = -xd[e];
        }
      }
      rv[i] = r;
    }
    if (stage) {
      const LDS double* xk = S.X + k * 8;
      double q8[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) q8[c] = 0.0;
      if (ld) {
        double qx = 0.0, qy = 0.0;
        for (int i = 0; i < m; ++i) {
          const double rg = sg[k * m + i] * ld[k * m + i];
          const double t = -rg;
          if (i < nb) {
            const int bi = boxidx(i);
#pragma unroll
            for (int c = 2; c < 8; ++c) q8[c] = c == bi ? t : q8[c];
          } else {
            const int o = i - nb;
            const double ddx = xk[0] - S.obx[o], ddy = xk[1] - S.oby[o];
            const double idd = rsq(ddx * ddx + ddy * ddy);
            qx += t * (-(ddx * idd));
            qy += t * (-(ddy * idd));
          }
        }
        q8[0] = qx;
        q8[1] = qy;
      }
      LDS double* qo = S.qs + k * 10;
#pragma unroll
      for (int c = 0; c < 8; ++c) qo[c] = q8[c];
    }
    sync();
    // 6. the solves: q and its state step
    S.resolve(rv);
    S.forward(dU, dX);
    if (io.q) {
      double* o = io.q + ((long long)b * io.na + d) * nwE;
      for (int i = lane; i < nw; i += WAVE) {
        const int e = ext_u(prm, i);
        if (e < 0) continue;
        o[e] = S.fixed(i) ? 0.0 : dU[i];
      }
    }
    // 7. J q, and y = sigma_s (lam_g_bar - J q) (stage 0's rows: J is zero there)
    {
      double* o = io.jq ? io.jq + ((long long)b * io.na + d) * ng : nullptr;
      for (int r = lane; r < ng; r += WAVE) {
        const double jq = r < m ? 0.0 : S.row_jd(r, dX);
        if (o) o[r] = jq;
        // (the difference first: on an active row sigma_s is large and J q close to lam_g_bar)
        yv[r] = ld ? sg[r] * (ld[r] - jq) : -(sg[r] * jq);
      }
    }
    if (!io.pbar) {
      sync();
      continue;
    }
    // 8. the pullback (nmpc_adjoint_kernel's steps 6 to 9 with z = -q, xi = -(dX/dw) q)
    double dx[8], du0 = 0.0;
#pragma unroll
    for (int c = 0; c < 8; ++c) dx[c] = k <= N ? -dX[k * 8 + c] : 0.0;
    if (k < N) du0 = S.fixed(k * 6) ? -0.0 : -dU[k * 6];
    double t0 = 0.0, t1 = 0.0;  // (Hl_k xi_k)[0:2]: the target's part of pbar
    if (k <= N) {
      double hs[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) hs[c] = 0.0;
      if (stage) {
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          double acc = 0.0;
#pragma unroll
          for (int q = 0; q < 6; ++q) acc += S.Hl[k * 21 + hp(a, q)] * dx[sv[q]];
          hs[sv[a]] = acc;
        }
        if (k < N) { t0 = hs[0]; t1 = hs[1]; }
        if (S.nobs > 0) {
          hs[0] += q00 * dx[0] + q01 * dx[1];
          hs[1] += q01 * dx[0] + q11 * dx[1];
        }
        // (stage N: no dynamics follow it, its terms are absent)
        hs[3] = k < N ? (d33 * dx[3] + d34 * dx[4]) + s03 * du0 : 0.0;
        hs[4] = k < N ? (d34 * dx[3] + d44 * dx[4]) + s04 * du0 : 0.0;
      } else {  // stage 0: Hxu_0 z_0 alone
        hs[3] = k < N ? s03 * du0 : 0.0;
        hs[4] = k < N ? s04 * du0 : 0.0;
      }
      if (Xd) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          if (c < nxE) hs[c] = hs[c] + Xd[k * nxE + c];
        }
      }
      GLB double* h = S.gl + k * 8;
#pragma unroll
      for (int c = 0; c < 8; ++c) h[c] = hs[c];
    }
    sync();
    // nu_k = s_k + G_k^T y_k + A_k^T nu_{k+1}
    S.adjoint(1.0, (const GLB double*)yv);
    // pbar, lane i forming internal entry i
    {
      double v = lane < 8 ? S.lam[lane] : 0.0;
      const double gxt = -wsum(t0);
      const double gyt = -wsum(t1);
      if (lane == 8) v = gxt;
      else if (lane == 9) v = gyt;
      if (w1p >= 0) {
        double a_ = 0.0;
        if (stage && k < N) {
#pragma unroll
          for (int a = 0; a < 6; ++a) a_ += uw[k * 12 + a] * dx[sv[a]];
        }
        const double s = wsum(a_);
        if (lane == w1p) v += s;
      }
      if (w2p >= 0) {
        double a_ = 0.0;
        if (stage && k < N) {
#pragma unroll
          for (int a = 0; a < 6; ++a) a_ += uw[k * 12 + 6 + a] * dx[sv[a]];
        }
        const double s = wsum(a_);
        if (lane == w2p) v += s;
      }
      for (int o = 0; o < S.nobs; ++o) {
        const int ix = prm->oxp[o], iy = prm->oyp[o];
        if (ix < 0 && iy < 0) continue;
        double cx = 0.0, cy = 0.0;
        if (k <= N) {  // row g = r_sum - |(x, y) - (ox, oy)|: dg/dox = (x - ox) / d
          const double yo = yv[k * m + nb + o];
          const LDS double* xk = S.X + k * 8;
          const double ddx = xk[0] - S.obx[o], ddy = xk[1] - S.oby[o];
          const double idd = rsq(ddx * ddx + ddy * ddy);
          cx = yo * (ddx * idd);
          cy = yo * (ddy * idd);
          if (stage) {  // the centre's move against the obstacle's own curvature, recomputed
            const double C = yb[k * m + nb + o];
            const double id3 = idd * idd * idd;
            const double h00 = C * (-ddy * ddy * id3), h01 = C * (ddx * ddy * id3), h11 = C * (-ddx * ddx * id3);
            cx -= h00 * dx[0] + h01 * dx[1];
            cy -= h01 * dx[0] + h11 * dx[1];
          }
        }
        cx = wsum(cx); cy = wsum(cy);
        if (lane == ix) v += cx;
        if (lane == iy) v += cy;
      }
      if (pe >= 0) io.pbar[((long long)b * io.na + d) * npE + pe] = v;
    }
    sync();
  }
}

}  // namespace

int nmpc_solve_adjoint_launch(const Params* dprm, int B, const SadjIO& io, void* stream) {
  hipLaunchKernelGGL(nmpc_solve_adjoint_kernel, dim3(B), dim3(WAVE), 0, (hipStream_t)stream, dprm, B, io);
  return (int)hipGetLastError();
}
