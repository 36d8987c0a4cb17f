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
// nmpc_solve_tangent.hip): the solver's own text throughout, and nmpc_solve_tangent.hip's LDS
// carve-up, workspace slices, weights, validity rules and ladder as they stand.
//
// Execution model: the siblings'.  One wavefront per scenario, fp64, stage k on lane k, rows
// and variables strided over the lanes, control flow wave-uniform.
// Once per wavefront:
//   1. nmpc_solve_tangent_kernel's steps 1 to 4, with s03, s04 in qs[8], qs[9] of stage 0;
//   2. lane k writes K_k (compacted to nu x nx, a fixed control's row 0.0), A_k, B_k and X*_k.
// Per direction (the factorisation is shared):
//   3. nmpc_solve_tangent_kernel's steps 5 to 10 and Solver::resolve;
//   4. kff = k - K xi, variables strided over the lanes, written through ext_u (a fixed
//      control's entry 0.0).
// Solver::forward, dlam_g and dX are not formed.
// (included by nmpc_eval.hip)

namespace {

static_assert(CapA::L.wstotal >= kSpolWs && CapB::L.wstotal >= kSpolWs && CapC::L.wstotal >= kSpolWs &&
                  CapD::L.wstotal >= kSpolWs && CapA32::L.wstotal >= kSpolWs && CapC32::L.wstotal >= kSpolWs &&
                  CapE::L.wstotal >= kSpolWs,
              "a solver class's workspace is smaller than one wavefront's of the policy kernel");

// LDS carve-up: nmpc_solve_tangent_kernel's
constexpr int PL_TOTAL = T_TOTAL;
static_assert(PL_TOTAL * 8 * 6 <= 160 * 1024, "policy kernel LDS: six workgroups per CU");

__global__ __launch_bounds__(WAVE) void nmpc_solve_policy_kernel(const Params* __restrict__ prm, int B, SpolIO io) {
  __shared__ __attribute__((aligned(16))) double smem[PL_TOTAL];
  const int b = blockIdx.x;
  if (b >= B) return;
  Solver<CapEv> S{};
  LDS double* sm = (LDS double*)smem;
  GLB double* gw = (GLB double*)(io.ws + (long long)b * kSpolWs);
  S.P = (const CST Params*)prm; S.sm = sm; S.lane_ = threadIdx.x; S.b = b;
  S.N = prm->N; S.m = prm->m; S.nobs = prm->nobs; S.nw = prm->nw; S.ng = prm->ng; S.T = prm->T;
  S.nb = prm->nb; S.nuE = prm->nuE; S.nwE = prm->nwE;
  S.U = gw + kKktU; S.gl = gw + kKktGl; S.Hl = gw + kKktHl; S.tc = gw + kKktTc; S.dc = gw + kKktDc;
  S.Qs = gw + kKktQs; S.K = gw + kKktK; S.Rk = gw + kKktRk; S.kf = gw + kKktKf;
  GLB double* Rd = gw + kKktRd;   // sigma_x, the kernel's layout
  GLB double* rv = gw + kKktRv;   // the direction's control terms
  GLB double* sg = gw + kStanSg;  // sigma_s
  GLB double* jpv = gw + kStanJp; // the direction's jp
  GLB double* uw = gw + kStanUw;  // after the ladder: unit-weight stage-cost gradients, 6 + 6 per stage
  GLB double* xw = gw + kStanXi;  // after the ladder: the direction's xi, 8 per stage
  S.pp = sm + A_PP; S.obx = sm + A_OB; S.oby = S.obx + NMPC_MAX_OBS; S.rvars = sm + A_RV; S.stamps = sm + A_ST;
  S.X = sm + A_X; S.trig = sm + A_TRIG; S.inc = sm + A_INC; S.lam = sm + A_LAM; S.qs = sm + A_QS;
  S.Pa = S.inc; S.Pb = S.inc + 64; S.pva = S.inc + 128; S.pvb = S.inc + 136;
  S.St = sm + A_SW; S.Rc = S.St + 48; S.Rv = S.Rc + 22;
  S.fixm = (LDS int*)(sm + A_FIX);
  LDS double* xi = sm + A_LAM;   // (dX/dp) dp, between steps 6 and 9 of nmpc_solve_tangent_kernel
  // lane k's copy of xi_k[0:2] moved for one obstacle row (nmpc_pproducts_kernel's dXo)
  LDS double* dXo = S.inc;
  LDS double* dpl = sm + T_DP;
  LDS double* cr = sm + T_CR;
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
  const double* db = io.dp ? io.dp + (long long)b * io.ld_dp : nullptr;
  const int nd = io.dp ? io.nd : 0;
  S.delta = 0.0;

  // every output of the scenario NaN (wave-uniform callers), its verdict and delta out
  auto finish_nan = [&](int verdict, double delta) {
    const long long nK = (long long)nuE * nxE * N, nA = (long long)nxE * nxE * N, nB = nK, nf = (long long)nd * nwE;
    if (io.K)
      for (long long i = lane; i < nK; i += WAVE) io.K[(long long)b * nK + i] = NAN;
    if (io.kff)
      for (long long i = lane; i < nf; i += WAVE) io.kff[(long long)b * nf + i] = NAN;
    if (io.A)
      for (long long i = lane; i < nA; i += WAVE) io.A[(long long)b * nA + i] = NAN;
    if (io.Bm)
      for (long long i = lane; i < nB; i += WAVE) io.Bm[(long long)b * nB + i] = NAN;
    if (io.X)
      for (long long i = lane; i < nXE; i += WAVE) io.X[(long long)b * nXE + i] = NAN;
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

  // ---------------- lane k: the second-order data of every direction's h_k, in registers
  // (nmpc_solve_tangent_kernel's; s03, s04 of stage 0 also feed its stage summary)
  double q00 = 0.0, q01 = 0.0, q11 = 0.0;
  double d33 = 0.0, d34 = 0.0, d44 = 0.0, s03 = 0.0, s04 = 0.0;
  double E03 = 0.0, E04 = 0.0, E13 = 0.0, E14 = 0.0, E23 = 0.0;
  {
    double b00 = 0.0, b10 = 0.0, b20 = 0.0;
    if (k < N) S.stage_AB(k, E03, E04, E13, E14, E23, b00, b10, b20);
  }
  if (k <= N) {  // lam_g-weighted obstacle curvature, rows in order
    const LDS double* xk = S.X + k * 8;
    for (int o = 0; o < S.nobs; ++o) {
      const double C = yb[k * m + nb + o];
      const double ddx = xk[0] - S.obx[o], ddy = xk[1] - S.oby[o];
      const double idd = rsq(ddx * ddx + ddy * ddy);
      const double id3 = idd * idd * idd;
      const double h00 = C * (-ddy * ddy * id3), h01 = C * (ddx * ddy * id3), h11 = C * (-ddx * ddx * id3);
      {
        // the rounded products summed, as nmpc_pproducts_kernel sums them (it also stores each
        // product, and its sum is not contracted into fused multiply-adds): the same bits
#pragma clang fp contract(off)
        q00 = q00 + h00; q01 = q01 + h01; q11 = q11 + h11;
      }
    }
  }
  if (k < N) {
    const LDS double* tg = S.trig + k * 8;
    const double ct = tg[0], stt = tg[1], cp = tg[2], sp = tg[3], v = tg[4];
    const LDS double* ln = S.lam + (k + 1) * 8;
    const double l0 = ln[0], l1 = ln[1], l2 = ln[2];
    d33 = T * (-l0 * v * cp * ct - l1 * v * sp * ct - l2 * v * stt);
    d44 = T * (-l0 * v * cp * ct - l1 * v * sp * ct);
    d34 = T * (l0 * v * sp * stt - l1 * v * cp * stt);
    s03 = T * (-l0 * cp * stt - l1 * sp * stt + l2 * ct);
    s04 = T * (-l0 * sp * ct + l1 * cp * ct);
  }

  // ---------------- the delta ladder: stage summaries (nmpc_kkt_kernel's text, and stage 0's
  // cross term) and factorisation
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
        } else {  // stage 0: S_0 alone (Q_0 stays 0), so that the stored K_0 is the stage's gain
          r03 = s03;
          r04 = s04;
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

  // ---------------- cost weights from p: unit-weight gradients, lane k stage k's, into the stage
  // summaries' slice (dead once the factorisation stands; the gradient slice is each direction's)
  if (w1p >= 0 || w2p >= 0) {
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

  // which entries of a direction something reads (lane i: internal entry i)
  bool reads = lane < 10;
  if (lane == w1p || lane == w2p) reads = true;
  for (int o = 0; o < S.nobs; ++o)
    if (lane == prm->oxp[o] || lane == prm->oyp[o]) reads = true;
  const int pe = lane < np ? ext_p(prm, lane) : -1;
  reads = reads && pe >= 0;
  sync();

  // ---------------- directions (step numbers: nmpc_solve_tangent_kernel's)
  for (int d = 0; d < nd; ++d) {
    // 5. the direction
    dpl[lane] = reads ? db[(long long)d * npE + pe] : 0.0;
    sync();
    // 6. state tangent of the parameters
    double dx[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) dx[c] = dpl[c];
    if (k < N) {
      S.inc[k * 8 + 5] = E03 * dx[3] + E04 * dx[4];
      S.inc[k * 8 + 6] = E13 * dx[3] + E14 * dx[4];
      S.inc[k * 8 + 7] = E23 * dx[3];
    }
    sync();
    if (k <= N) {
      for (int j = 0; j < k; ++j) {
        dx[0] = dx[0] + S.inc[j * 8 + 5];
        dx[1] = dx[1] + S.inc[j * 8 + 6];
        dx[2] = dx[2] + S.inc[j * 8 + 7];
      }
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        xi[k * 8 + c] = dx[c];
        xw[k * 8 + c] = dx[c];
      }
    }
    // 7. h_k, and the cross term of step 10
    if (k <= N) {
      GLB double* h = S.gl + k * 8;
      double hs[6];
#pragma unroll
      for (int a = 0; a < 6; ++a) hs[a] = 0.0;
      if (k < N) {
        // the stage cost sees the target's move as the opposite move of (x, y)
        const double xs[6] = {dx[0] - dpl[8], dx[1] - dpl[9], dx[2], dx[5], dx[6], dx[7]};
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          double acc = 0.0;
#pragma unroll
          for (int q = 0; q < 6; ++q) acc += S.Hl[k * 21 + hp(a, q)] * xs[q];
          hs[a] = acc;
        }
        if (w1p >= 0) {
          const double s = dpl[w1p];
#pragma unroll
          for (int a = 0; a < 6; ++a) hs[a] += s * uw[k * 12 + a];
        }
        if (w2p >= 0) {
          const double s = dpl[w2p];
#pragma unroll
          for (int a = 0; a < 6; ++a) hs[a] += s * uw[k * 12 + 6 + a];
        }
      }
      if (S.nobs > 0) {
        hs[0] += q00 * dx[0] + q01 * dx[1];
        hs[1] += q01 * dx[0] + q11 * dx[1];
        for (int o = 0; o < S.nobs; ++o) {  // an obstacle's own move, against its own curvature
          const int ix = prm->oxp[o], iy = prm->oyp[o];
          if (ix < 0 && iy < 0) continue;
          const LDS double* xk = S.X + k * 8;
          const double C = yb[k * m + nb + o];
          const double ddx = xk[0] - S.obx[o], ddy = xk[1] - S.oby[o];
          const double idd = rsq(ddx * ddx + ddy * ddy);
          const double id3 = idd * idd * idd;
          const double h00 = C * (-ddy * ddy * id3), h01 = C * (ddx * ddy * id3), h11 = C * (-ddx * ddx * id3);
          if (ix >= 0) { hs[0] -= h00 * dpl[ix]; hs[1] -= h01 * dpl[ix]; }
          if (iy >= 0) { hs[0] -= h01 * dpl[iy]; hs[1] -= h11 * dpl[iy]; }
        }
      }
#pragma unroll
      for (int a = 0; a < 6; ++a) h[sv[a]] = hs[a];
      // (stage N: no dynamics follow it, its terms are absent)
      h[3] = k < N ? d33 * dx[3] + d34 * dx[4] : 0.0;
      h[4] = k < N ? d34 * dx[3] + d44 * dx[4] : 0.0;
      cr[k] = k < N ? s03 * dx[3] + s04 * dx[4] : 0.0;
    }
    sync();
    // 8. jp = (dg/dp) dp, lane k its stage's rows
    if (k <= N) {
      for (int i = 0; i < m; ++i) {
        const int r = k * m + i;
        if (i < nb) {
          jpv[r] = S.row_jd(r, xi);
        } else {  // the row sees its obstacle's move as the opposite move of (x, y)
          const int ix = prm->oxp[i - nb], iy = prm->oyp[i - nb];
          dXo[k * 8] = ix >= 0 ? dx[0] - dpl[ix] : dx[0];
          dXo[k * 8 + 1] = iy >= 0 ? dx[1] - dpl[iy] : dx[1];
          jpv[r] = S.row_jd(r, dXo);
        }
      }
    }
    sync();  // xi leaves the multipliers' buffer
    // 9. mu_k = h_k + A_k^T mu_{k+1}
    S.adjoint(1.0, (const double*)nullptr);
    // 10. r_k = hp, q_k = G_k^T (sigma_s jp)
    for (int i = lane; i < nw; i += WAVE) {
      const int e = ext_u(prm, i);
      double r = 0.0;
      if (e >= 0) {
        const int kk = i / 6;
        const double g = S.grad_u(i);
        r = i == 6 * kk ? g + cr[kk] : g;
      }
      rv[i] = r;
    }
    if (k >= 1 && k <= N) {
      const LDS double* xk = S.X + k * 8;
      double q8[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) q8[c] = 0.0;
      double qx = 0.0, qy = 0.0;
      for (int i = 0; i < m; ++i) {
        const double t = sg[k * m + i] * jpv[k * m + i];
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
      LDS double* qo = S.qs + k * 10;
#pragma unroll
      for (int c = 0; c < 8; ++c) qo[c] = q8[c];
    }
    sync();
    // the solve's backward half: k_k
    S.resolve(rv);
    // kff = k - K xi (xi_k as lane k stored it in step 6)
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
