// nmpc_point.hip -- what the kernels that work at a solve's point (x*, lam_g*, lam_x*) share:
// the fused reverse-mode sensitivity (nmpc_solve_adjoint.hip), the fused forward-mode
// sensitivity (nmpc_solve_tangent.hip) and the feedback policy (nmpc_solve_policy.hip).  Each of
// them is the sequence
//   point_bind, load_params, load_controls, point_rollout, point_weights (info = -11),
//   point_derivs, [its own second-order data], point_ladder (info = 1), point_verdict,
//   point_unit_grads,
// then its own per-seed or per-direction work; the tangent and policy kernels also share
// point_curvature, point_reads and point_direction_rhs.  The LDS head, bind_solver, the scenario
// load, point_rollout, point_dyn2, point_summary and point_reads are nmpc_eval_shared.hip's, shared
// with the kernels at given points; point_unit_grads, point_curvature and point_direction_rhs keep
// their own text for the unit-weight gradients, the obstacle curvature, the tangent and q_k: on
// the shared helpers the three kernels' instructions changed and two of them measured slower
// (DESIGN.md 26).
//
// Part of the evaluation kernel's translation unit (nmpc_eval.hip includes this file after
// nmpc_adjoint.hip and before nmpc_solve_adjoint.hip), so everything is the text the solver
// compiles: Solver::rollout, stage_cost, row_value, derivs, adjoint, riccati, stage_AB, grad_u,
// row_jd.  Every function is forced inline: a kernel's instructions are those of the text
// written out in it.
//
// Execution model: the siblings'.  One wavefront per scenario, fp64, stage k on lane k, rows
// and variables strided over the lanes, control flow wave-uniform.
// (included by nmpc_eval.hip)

namespace {

static_assert(fits_every_class(kPointWs),
              "a solver class's workspace is smaller than one wavefront's of a solution-point kernel");
static_assert(kPointXi + 8 * kEvalStages <= kKktK, "the unit-weight gradients and xi live in the stage summaries' slice");

// LDS carve-up (doubles): the KKT kernel's without a buffer of its own for the state step, which
// lives in the prefix-sum scratch: Solver::forward reads nothing there, every lane takes its
// stage's entries into registers before the pullback's sweep uses the scratch again, and the
// next seed's sweeps find it dead.  23.6 KB: six workgroups per CU's 160 KiB, where the KKT
// kernel's 27.7 KB allow five
constexpr int A_QS = B_END;                   // q_k (8), S_k[0][3], S_k[0][4] per stage
constexpr int A_SW = A_QS + 10 * NS;          // S~ (48), R~ (22), r~ (8) of the current stage
constexpr int A_FIX = A_SW + 48 + 22 + 8;     // fixed-control masks, one int per stage
constexpr int A_TOTAL = A_FIX + NS / 2 + 2;
static_assert(A_TOTAL * 8 <= 32 * 1024, "fused sensitivity kernel LDS");
// the tangent and policy kernels': then the direction and the cross term of point_direction_rhs.
// 24.6 KB: six workgroups per CU's 160 KiB still
constexpr int T_DP = A_TOTAL;      // the direction, internal p layout (<= 64)
constexpr int T_CR = T_DP + 64;    // the direction's Hxu_k^T xi_k
constexpr int T_TOTAL = T_CR + NS;
static_assert(T_TOTAL * 8 * 6 <= 160 * 1024, "fused tangent and policy kernel LDS: six workgroups per CU");

// numpy.maximum: a NaN operand stays (fmax would drop it)
__device__ __forceinline__ double npmax(double a, double b) { return (a != a || b != b) ? NAN : (a > b ? a : b); }
// Solver.barrier_weights' weight of one value between its bounds
__device__ __forceinline__ double barrier_sigma(double v, double lam, double lo, double hi, double brf) {
  const double sl = npmax(v - lo, brf * npmax(1.0, fabs(lo)));
  const double su = npmax(hi - v, brf * npmax(1.0, fabs(hi)));
  return npmax(-lam, 0.0) / sl + npmax(lam, 0.0) / su;
}
// n doubles at o NaN, strided over the lanes (a null o: nothing)
__device__ __forceinline__ void nan_fill(double* o, long long n, int lane) {
  if (o)
    for (long long i = lane; i < n; i += WAVE) o[i] = NAN;
}

// the scenario's rows of the nine point inputs and its workspace slices
struct PointRefs {
  const double *xb, *yb, *lxb, *gb, *lbxb, *ubxb, *lbgb, *ubgb;
  GLB double* Rd;  // sigma_x, the kernel's layout
  GLB double* rv;  // the seed's or direction's control terms
  GLB double* dU;  // its step
  GLB double* sg;  // sigma_s
  GLB double* yv;  // the seed's y, or the direction's jp
  GLB double* uw;  // after the ladder: unit-weight stage-cost gradients, 6 + 6 per stage
  GLB double* xw;  // after the ladder: the direction's xi, 8 per stage
};

// the solver onto the LDS carve-up above and the scenario's workspace slices
__device__ __forceinline__ PointRefs point_bind(Solver<CapEv>& S, const Params* __restrict__ prm, LDS double* sm,
                                                const PointIO& io, int b) {
  GLB double* gw = (GLB double*)(io.ws + (long long)b * kPointWs);
  bind_solver(S, prm, sm, gw, b, kKktU, kKktGl, kKktHl, kKktTc, kKktDc);
  S.Qs = gw + kKktQs; S.K = gw + kKktK; S.Rk = gw + kKktRk; S.kf = gw + kKktKf;
  S.qs = sm + A_QS;
  S.Pa = S.inc; S.Pb = S.inc + 64; S.pva = S.inc + 128; S.pvb = S.inc + 136;
  S.St = sm + A_SW; S.Rc = S.St + 48; S.Rv = S.Rc + 22;
  S.fixm = (LDS int*)(sm + A_FIX);
  S.delta = 0.0;
  PointRefs R;
  R.xb = io.x + (long long)b * io.ld_x;
  R.yb = io.lam_g + (long long)b * io.ld_lam_g;
  R.lxb = io.lam_x + (long long)b * io.ld_lam_x;
  R.gb = io.g ? io.g + (long long)b * io.ld_g : nullptr;
  R.lbxb = io.lbx + (long long)b * io.ld_lbx;
  R.ubxb = io.ubx + (long long)b * io.ld_ubx;
  R.lbgb = io.lbg + (long long)b * io.ld_lbg;
  R.ubgb = io.ubg + (long long)b * io.ld_ubg;
  R.Rd = gw + kKktRd; R.rv = gw + kKktRv; R.dU = gw + kKktDu;
  R.sg = gw + kPointSg; R.yv = gw + kPointY; R.uw = gw + kPointUw; R.xw = gw + kPointXi;
  return R;
}

// the barrier weights, Solver.barrier_weights' operations in their order:
//   sl = max(v - lo, brf max(1, |lo|)), su = max(hi - v, brf max(1, |hi|)),
//   sigma = max(-lam, 0) / sl + max(lam, 0) / su
// (max as numpy.maximum: a NaN stays); lane k its stage's controls (lbx == ubx: +inf, the
// variable leaves the system, Solver::fixm) and its stage's rows (v = the given g, else the
// kernel's own row value).  True, wave-uniform, on an equality row, lbx > ubx or a weight that
// is not a finite non-negative number: the caller ends the scenario with info = -11
__device__ __forceinline__ bool point_weights(Solver<CapEv>& S, const Params* __restrict__ prm, const PointRefs& R,
                                           int k) {
  const int N = S.N, m = S.m, nuE = S.nuE;
  const double brf = prm->o.bound_relax_factor;
  bool bad = false;
  int fmk = 0;
  if (k < N) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double v = 0.0;
      if (c < nuE) {
        const int e = k * nuE + c;
        const double lo = R.lbxb[e], hi = R.ubxb[e];
        v = lo == hi ? INFINITY : barrier_sigma(R.xb[e], R.lxb[e], lo, hi, brf);
        bad |= lo > hi;
      }
      const bool fx = v == INFINITY;
      bad |= !(v >= 0.0);
      fmk |= fx ? (1 << c) : 0;
      R.Rd[k * 6 + c] = fx ? 0.0 : v;
      R.rv[k * 6 + c] = 0.0;
    }
  }
  if (k <= N) {
    S.fixm[k] = fmk;
    const LDS double* xk = S.X + k * 8;
    for (int i = 0; i < m; ++i) {
      const int r = k * m + i;
      const double lo = R.lbgb[r], hi = R.ubgb[r];
      const double v = barrier_sigma(R.gb ? R.gb[r] : S.row_value(xk, i), R.yb[r], lo, hi, brf);
      bad |= lo == hi || !(v >= 0.0) || v == INFINITY;
      R.sg[r] = v;
    }
  }
  S.nfix = wany(fmk != 0) ? 1 : 0;
  return wany(bad);
}

// derivatives and multipliers at the scenario's own weights: gl, Hl, lam_{k+1} (the objective
// factor is 1)
__device__ __forceinline__ void point_derivs(Solver<CapEv>& S, const PointRefs& R) {
  S.derivs<true, true>(S.X, S.U, S.tc);
  S.adjoint(1.0, R.yb);
}

// the delta ladder: delta = 0, the stage summaries with D = sigma_s + delta, Solver::riccati; on
// a failed inertia verdict the next rung (first_hessian_perturbation, then
// x perturb_inc_fact_first, then x perturb_inc_fact: the host ladder's multiplications) while it
// is <= max_hessian_perturbation; c03, c04 as point_summary's.  Returns the verdict (0, or 1 beyond the last rung: the caller
// ends the scenario with info = 1) and leaves the last delta tried in `delta`
__device__ __forceinline__ int point_ladder(Solver<CapEv>& S, const Params* __restrict__ prm, const PointRefs& R,
                                            int k, double c03, double c04, double& delta) {
  const double first = prm->o.first_hessian_perturbation, inc_first = prm->o.perturb_inc_fact_first;
  const double inc = prm->o.perturb_inc_fact, dmax = prm->o.max_hessian_perturbation;
  delta = 0.0;
  // (weights and multipliers are given here: point_summary's null checks fold away)
  const double *sg = (const double*)R.sg, *yb = R.yb;
  __builtin_assume(sg != nullptr);
  __builtin_assume(yb != nullptr);
  while (true) {
    S.delta = delta;
    point_summary(S, k, 1.0, sg, yb, delta, c03, c04);
    sync();
    if (S.riccati(R.Rd, R.rv)) return 0;  // zero linear terms
    sync();
    // the next rung, by the host ladder's multiplications
    const double nxt = delta == 0.0 ? first : (delta == first ? inc_first * delta : inc * delta);
    if (!(nxt <= dmax) || !(nxt > delta)) return 1;  // (a ladder that does not climb ends here too)
    delta = nxt;
  }
}

// the scenario's verdict and delta out
__device__ __forceinline__ void point_verdict(const Solver<CapEv>& S, const PointIO& io, int lane, int verdict,
                                              double delta) {
  if (lane == 0) {
    if (io.info) io.info[S.b] = verdict;
    if (io.delta) io.delta[S.b] = delta;
  }
}

// cost weights from p: unit-weight stage-cost gradients, lane k stage k's, into the stage
// summaries' slice (dead once the factorisation stands; the gradient slice is each seed's or
// direction's)
__device__ __forceinline__ void point_unit_grads(Solver<CapEv>& S, const Params* __restrict__ prm, const PointRefs& R,
                                                 int lane) {
  const int w1p = prm->w1p, w2p = prm->w2p;
  if (w1p < 0 && w2p < 0) return;
  const int k = lane, N = S.N;
  const int sv[6] = {0, 1, 2, 5, 6, 7};  // the states a stage cost reads
  const double w1s = S.rvars[30], w2s = S.rvars[31];
  sync();
  if (w1p >= 0) {
    if (lane == 0) { S.rvars[30] = 1.0; S.rvars[31] = 0.0; }
    sync();
    S.derivs<false, true>(S.X, S.U, S.tc);
    if (k < N) {
#pragma unroll
      for (int a = 0; a < 6; ++a) R.uw[k * 12 + a] = S.gl[k * 8 + sv[a]];
    }
  }
  if (w2p >= 0) {
    if (lane == 0) { S.rvars[30] = 0.0; S.rvars[31] = 1.0; }
    sync();
    S.derivs<false, true>(S.X, S.U, S.tc);
    if (k < N) {
#pragma unroll
      for (int a = 0; a < 6; ++a) R.uw[k * 12 + 6 + a] = S.gl[k * 8 + sv[a]];
    }
  }
  if (lane == 0) { S.rvars[30] = w1s; S.rvars[31] = w2s; }
  sync();
}

// ---- the tangent and policy kernels' directions

// lane k: the second-order data of every direction's h_k, in registers (nmpc_pproducts_kernel's
// step 4 without the per-obstacle curvature in the workspace; stage 0 included, its
// xi_0 = dp[0:nx] is not zero): the summed obstacle curvature, the dynamics terms and the
// entries of A_k = I + E_k
struct PointCurv {
  double q00 = 0.0, q01 = 0.0, q11 = 0.0;
  double d33 = 0.0, d34 = 0.0, d44 = 0.0, s03 = 0.0, s04 = 0.0;
  double E03 = 0.0, E04 = 0.0, E13 = 0.0, E14 = 0.0, E23 = 0.0;
};
__device__ __forceinline__ PointCurv point_curvature(Solver<CapEv>& S, const PointRefs& R, int k) {
  const int N = S.N, m = S.m, nb = S.nb;
  const double T = S.T;
  PointCurv c;
  {
    double b00 = 0.0, b10 = 0.0, b20 = 0.0;
    if (k < N) S.stage_AB(k, c.E03, c.E04, c.E13, c.E14, c.E23, b00, b10, b20);
  }
  if (k <= N) {  // lam_g-weighted obstacle curvature, rows in order
    const LDS double* xk = S.X + k * 8;
    for (int o = 0; o < S.nobs; ++o) {
      const double C = R.yb[k * m + nb + o];
      const double ddx = xk[0] - S.obx[o], ddy = xk[1] - S.oby[o];
      const double idd = rsq(ddx * ddx + ddy * ddy);
      const double id3 = idd * idd * idd;
      const double h00 = C * (-ddy * ddy * id3), h01 = C * (ddx * ddy * id3), h11 = C * (-ddx * ddx * id3);
      {
        // the rounded products summed, as nmpc_pproducts_kernel sums them (it also stores each
        // product, and its sum is not contracted into fused multiply-adds): the same bits
#pragma clang fp contract(off)
        c.q00 = c.q00 + h00; c.q01 = c.q01 + h01; c.q11 = c.q11 + h11;
      }
    }
  }
  if (k < N) {  // rounded products (the ladder's summaries fuse theirs into Q)
    const Dyn2 e = point_dyn2(S, k);
    c.d33 = T * e.e33;
    c.d44 = T * e.e44;
    c.d34 = T * e.e34;
    c.s03 = T * e.e03;
    c.s04 = T * e.e04;
  }
  return c;
}

// one direction dd of the parameters up to the sync() before Solver::resolve:
// nmpc_pproducts_kernel's steps 6 to 11 feeding nmpc_kkt_kernel's step 6
//   5. the entries of the direction that something reads, to LDS in the kernel's p layout;
//   6. xi = (dX/dp) dp by in-order prefix sums, into the multipliers' LDS buffer (lam is dead
//      once the ladder has stood; the sweep of step 9 rewrites the buffer) and, lane k its
//      stage's, into the workspace (R.xw) for the caller;
//   7. h_k, the stage cost's Hessian read from the workspace (the objective factor is 1) and an
//      obstacle's own curvature lam_{k,o} Hg_o recomputed where its centre comes from p;
//   8. jp, lane k its stage's rows, into the workspace (R.yv);
//   9. mu_k = h_k + A_k^T mu_{k+1} (Solver::adjoint);
//  10. r_k = hp = B_k^T mu_{k+1} + Hxu_k^T xi_k (the negation of -hp that the recursion's sign
//      convention asks for is exact, so it is not formed), q_k = G_k^T (sigma_s jp): one
//      product per row, the host route's
__device__ __forceinline__ void point_direction_rhs(Solver<CapEv>& S, const Params* __restrict__ prm,
                                                    const PointRefs& R, int lane, const PointCurv& cv,
                                                    const double* dd, bool reads, int pe) {
  const int k = lane, N = S.N, m = S.m, nb = S.nb, nw = S.nw;
  const int w1p = prm->w1p, w2p = prm->w2p;
  const int sv[6] = {0, 1, 2, 5, 6, 7};  // the states a stage cost reads
  LDS double* xi = S.lam;        // (dX/dp) dp, between steps 6 and 9
  // lane k's copy of xi_k[0:2] moved for one obstacle row (nmpc_pproducts_kernel's dXo)
  LDS double* dXo = S.inc;
  LDS double* dpl = S.sm + T_DP;
  LDS double* cr = S.sm + T_CR;
  GLB double* jpv = R.yv;
  // 5. the direction
  dpl[lane] = reads ? dd[pe] : 0.0;
  sync();
  // 6. state tangent of the parameters
  double dx[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) dx[c] = dpl[c];
  if (k < N) {
    S.inc[k * 8 + 5] = cv.E03 * dx[3] + cv.E04 * dx[4];
    S.inc[k * 8 + 6] = cv.E13 * dx[3] + cv.E14 * dx[4];
    S.inc[k * 8 + 7] = cv.E23 * dx[3];
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
      R.xw[k * 8 + c] = dx[c];
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
        for (int a = 0; a < 6; ++a) hs[a] += s * R.uw[k * 12 + a];
      }
      if (w2p >= 0) {
        const double s = dpl[w2p];
#pragma unroll
        for (int a = 0; a < 6; ++a) hs[a] += s * R.uw[k * 12 + 6 + a];
      }
    }
    if (S.nobs > 0) {
      hs[0] += cv.q00 * dx[0] + cv.q01 * dx[1];
      hs[1] += cv.q01 * dx[0] + cv.q11 * dx[1];
      for (int o = 0; o < S.nobs; ++o) {  // an obstacle's own move, against its own curvature
        const int ix = prm->oxp[o], iy = prm->oyp[o];
        if (ix < 0 && iy < 0) continue;
        const LDS double* xk = S.X + k * 8;
        const double C = R.yb[k * m + nb + o];
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
    h[3] = k < N ? cv.d33 * dx[3] + cv.d34 * dx[4] : 0.0;
    h[4] = k < N ? cv.d34 * dx[3] + cv.d44 * dx[4] : 0.0;
    cr[k] = k < N ? cv.s03 * dx[3] + cv.s04 * dx[4] : 0.0;
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
    R.rv[i] = r;
  }
  if (k >= 1 && k <= N) {
    const LDS double* xk = S.X + k * 8;
    double q8[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) q8[c] = 0.0;
    double qx = 0.0, qy = 0.0;
    for (int i = 0; i < m; ++i) {
      const double t = R.sg[k * m + i] * jpv[k * m + i];
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
}

}  // namespace
