// nmpc_eval_shared.hip -- what the kernels of the evaluation unit share: the five kernels at
// given points (nmpc_eval.hip, nmpc_products.hip, nmpc_kkt.hip, nmpc_pproducts.hip,
// nmpc_adjoint.hip), the steps of the three kernels at a solve's point (nmpc_point.hip) and the
// scenario load of the two policy-rollout kernels.  No kernel of its own: the head of the LDS
// carve-up, the workspace check, the solver's binding, the scenario load, the rollout, the
// unit-weight stage-cost gradients, the second-order data of a stage (dynamics terms, one
// obstacle's curvature, the stage summary), q_k = G_k^T t and the output loops.  What stays a copy
// in a kernel, because sharing it moved a bit of that kernel's output (the compiler orders the
// operands of a sum, and so chooses the product it fuses, by the position of the code around it) or
// changed the instructions of a kernel that then measured slower, is listed in DESIGN.md 26.
//
// Part of the evaluation kernel's translation unit: nmpc_eval.hip includes this file right after
// nmpc_eval.h and before its own kernel, so everything is the text the solver compiles.  Every
// function is forced inline on Solver<CapEv>&: a kernel's instructions are those of the text
// written out in it.  Where two kernels round a sum differently (a product added into a sum may
// contract to a fused multiply-add, an assigned product may not) the helper returns the terms and
// the summation statement stays with the caller.
// (included by nmpc_eval.hip)

namespace {

// ---- LDS: the head every carve-up of the unit's wavefront-per-scenario kernels starts with
// (doubles); each kernel's own buffers follow from B_END
constexpr int NS = kEvalStages;
constexpr int B_PP = 0;                       // p, internal layout (<= 64)
constexpr int B_OB = B_PP + 64;               // obstacle x (16), y (16)
constexpr int B_RV = B_OB + 2 * NMPC_MAX_OBS; // Solver::rvars; [30], [31] = cost weights
constexpr int B_ST = B_RV + 32;               // phase-timer slots (NMPC_STAMPS builds write them)
constexpr int B_X = B_ST + PH_COUNT;          // trajectory, 8 per stage
constexpr int B_TRIG = B_X + 8 * NS;
constexpr int B_INC = B_TRIG + 8 * NS;        // prefix / suffix sum scratch
constexpr int B_LAM = B_INC + 8 * NS;         // lam, then each direction's or seed's multipliers
constexpr int B_END = B_LAM + 8 * NS;

// every solver class's workspace covers ws doubles: a handle whose workspace covers B for a solve
// covers B wavefronts of a kernel that takes ws each
constexpr bool fits_every_class(int ws) {
  return CapA::L.wstotal >= ws && CapB::L.wstotal >= ws && CapC::L.wstotal >= ws && CapD::L.wstotal >= ws &&
         CapA32::L.wstotal >= ws && CapC32::L.wstotal >= ws && CapE::L.wstotal >= ws;
}

// the solver onto the LDS head above and onto the slices U, gl, Hl, tc, dc of the wavefront's
// workspace gw (offsets in doubles)
__device__ __forceinline__ void bind_solver(Solver<CapEv>& S, const Params* __restrict__ prm, LDS double* sm,
                                            GLB double* gw, int b, int oU, int oGl, int oHl, int oTc, int oDc) {
  S.P = (const CST Params*)prm; S.sm = sm; S.lane_ = threadIdx.x; S.b = b;
  S.N = prm->N; S.m = prm->m; S.nobs = prm->nobs; S.nw = prm->nw; S.ng = prm->ng; S.T = prm->T;
  S.nb = prm->nb; S.nuE = prm->nuE; S.nwE = prm->nwE;
  S.U = gw + oU; S.gl = gw + oGl; S.Hl = gw + oHl; S.tc = gw + oTc; S.dc = gw + oDc;
  S.pp = sm + B_PP; S.obx = sm + B_OB; S.oby = S.obx + NMPC_MAX_OBS; S.rvars = sm + B_RV; S.stamps = sm + B_ST;
  S.X = sm + B_X; S.trig = sm + B_TRIG; S.inc = sm + B_INC; S.lam = sm + B_LAM;
}

// ---- scenario data (as solve_one loads it)

// None of the pieces synchronises: a sync() stands between load_p and the two that read p from
// LDS, and the caller's sync() follows the last of them.

// p (the scenario's row pb) to LDS in the internal layout
__device__ __forceinline__ void load_p(Solver<CapEv>& S, const Params* __restrict__ prm, int lane, const double* pb) {
  for (int i = lane; i < prm->np; i += WAVE) {
    const int e = ext_p(prm, i);
    S.pp[i] = e >= 0 ? pb[e] : 0.0;
  }
}
// obstacle centres, from p or the model's constants
__device__ __forceinline__ void load_obstacles(Solver<CapEv>& S, const Params* __restrict__ prm, int lane) {
  if (lane < NMPC_MAX_OBS) {
    const bool on = lane < S.nobs;
    S.obx[lane] = on ? (prm->oxp[lane] >= 0 ? S.pp[prm->oxp[lane]] : prm->ox[lane]) : 0.0;
    S.oby[lane] = on ? (prm->oyp[lane] >= 0 ? S.pp[prm->oyp[lane]] : prm->oy[lane]) : 0.0;
  }
}
// cost weights, from p or the model's constants
__device__ __forceinline__ void load_weights(Solver<CapEv>& S, const Params* __restrict__ prm, int lane) {
  if (lane == 0) {
    S.rvars[30] = prm->w1p >= 0 ? S.pp[prm->w1p] : prm->w1;
    S.rvars[31] = prm->w2p >= 0 ? S.pp[prm->w2p] : prm->w2;
  }
}
// the parameter half: stamps, p, obstacle centres and cost weights to LDS (one sync() inside, after
// p).  The caller's sync() follows (after load_controls where there are controls)
__device__ __forceinline__ void load_params(Solver<CapEv>& S, const Params* __restrict__ prm, int lane,
                                            const double* pb) {
  if (lane < PH_COUNT) S.stamps[lane] = 0.0;
  load_p(S, prm, lane, pb);
  sync();
  load_obstacles(S, prm, lane);
  load_weights(S, prm, lane);
}
// the control half: the controls of xb to the workspace in the kernel's 6-per-stage layout (the
// no-gimbal model's absent controls are 0) and, where an adjoint with rows follows, their unit
// scaling
__device__ __forceinline__ void load_controls(Solver<CapEv>& S, const Params* __restrict__ prm, int lane,
                                              const double* xb, bool unit_rows) {
  for (int i = lane; i < S.nw; i += WAVE) {
    const int e = ext_u(prm, i);
    S.U[i] = e >= 0 ? xb[e] : 0.0;
  }
  if (unit_rows)
    for (int r = lane; r < S.ng; r += WAVE) S.dc[r] = 1.0;  // unscaled rows
}

// rollout and stage costs (their transcendentals, the cache that derivs<., true> reads)
__device__ __forceinline__ void point_rollout(Solver<CapEv>& S, int lane) {
  S.rollout(S.U, S.X);
  if (lane < S.N) (void)S.stage_cost(S.X + lane * 8, S.tc + lane * 12);
  sync();
}

// cost weights from p: the stage-cost gradients with the weights (1, 0) and (0, 1) (derivs<false,
// true> on the swapped weights, as the solve's lam_p block forms the unit-weight costs), lane k
// stage k's.  put(s, g): entry a of the (1, 0) gradient over the states a stage cost reads as
// s = a, of the (0, 1) gradient as s = 6 + a.  (nmpc_adjoint_kernel's; nmpc_pproducts_kernel, which
// also takes the unit-weight costs, and nmpc_point.hip's point_unit_grads keep their text)
template <class Put>
__device__ __forceinline__ void unit_weight_grads(Solver<CapEv>& S, const Params* __restrict__ prm, int lane,
                                                  Put put) {
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
      for (int a = 0; a < 6; ++a) put(a, S.gl[k * 8 + sv[a]]);
    }
  }
  if (w2p >= 0) {
    if (lane == 0) { S.rvars[30] = 0.0; S.rvars[31] = 1.0; }
    sync();
    S.derivs<false, true>(S.X, S.U, S.tc);
    if (k < N) {
#pragma unroll
      for (int a = 0; a < 6; ++a) put(6 + a, S.gl[k * 8 + sv[a]]);
    }
  }
  if (lane == 0) { S.rvars[30] = w1s; S.rvars[31] = w2s; }
  sync();
}

// ---- a stage's second-order data

// the entries of A_k = I + E_k and of B_k's first column, stage k < N on lane k (zeros elsewhere)
struct StageAB { double E03 = 0.0, E04 = 0.0, E13 = 0.0, E14 = 0.0, E23 = 0.0, b00 = 0.0, b10 = 0.0, b20 = 0.0; };
__device__ __forceinline__ StageAB point_stage_ab(Solver<CapEv>& S, int k) {
  StageAB a;
  if (k < S.N) S.stage_AB(k, a.E03, a.E04, a.E13, a.E14, a.E23, a.b00, a.b10, a.b20);
  return a;
}

// second derivatives of lam_{k+1}^T T f(x_k, u_k) before the factor T (Solver::assemble's dyn
// branch), stage k < N on lane k: the three entries of d2_xx and S_k's two.  Two uses, two
// roundings: a stage summary adds T * e into Q (a fused multiply-add), every other use assigns
// T * e (a rounded product)
struct Dyn2 { double e33, e44, e34, e03, e04; };
__device__ __forceinline__ Dyn2 point_dyn2(const Solver<CapEv>& S, int k) {
  const LDS double* tg = S.trig + k * 8;
  const double ct = tg[0], stt = tg[1], cp = tg[2], sp = tg[3], v = tg[4];
  const LDS double* ln = S.lam + (k + 1) * 8;
  const double l0 = ln[0], l1 = ln[1], l2 = ln[2];
  Dyn2 e;
  e.e33 = -l0 * v * cp * ct - l1 * v * sp * ct - l2 * v * stt;
  e.e44 = -l0 * v * cp * ct - l1 * v * sp * ct;
  e.e34 = l0 * v * sp * stt - l1 * v * cp * stt;
  e.e03 = -l0 * cp * stt - l1 * sp * stt + l2 * ct;
  e.e04 = -l0 * sp * ct + l1 * cp * ct;
  return e;
}

// stage k's (x, y) against obstacle o's centre, and the reciprocal of their distance
struct ObsGeo { double ddx, ddy, idd; };
__device__ __forceinline__ ObsGeo obstacle_geo(const Solver<CapEv>& S, int k, int o) {
  const LDS double* xk = S.X + k * 8;
  ObsGeo d;
  d.ddx = xk[0] - S.obx[o];
  d.ddy = xk[1] - S.oby[o];
  d.idd = rsq(d.ddx * d.ddx + d.ddy * d.ddy);
  return d;
}
// one obstacle row's curvature C Hg_o at stage k, its entries (x, x), (x, y), (y, y): rounded
// products.  How they are summed (contracted into the sum or not, over which stages) is the
// caller's statement
struct ObsCurv { double h00, h01, h11; };
__device__ __forceinline__ ObsCurv obstacle_curvature(const ObsGeo& d, double C) {
  const double id3 = d.idd * d.idd * d.idd;
  ObsCurv h;
  h.h00 = C * (-d.ddy * d.ddy * id3);
  h.h01 = C * (d.ddx * d.ddy * id3);
  h.h11 = C * (-d.ddx * d.ddx * id3);
  return h;
}
__device__ __forceinline__ ObsCurv obstacle_curvature(const Solver<CapEv>& S, int k, int o, double C) {
  return obstacle_curvature(obstacle_geo(S, k, o), C);
}

// lane k <= N: the stage summary Q_k = obj_factor Hl_k + G_k^T (sigma_s + delta) G_k
// + sum_o lam_{k,o} Hg_o + the dynamics terms of lam_{k+1}^T T f, and S_k's two entries -- the
// expressions of Solver::assemble's Newton mode with D = sigma_s + delta, for k >= 1 (stage 0 is
// constant in w: Q_0 = 0); the linear terms zero.  sg and yb may be null (weights, multipliers
// of 0).  c03, c04: stage 0's S_0 where it enters too, so that the stored K_0 is the stage's gain
// (the policy kernel's; 0.0 elsewhere)
__device__ __forceinline__ void point_summary(Solver<CapEv>& S, int k, double obj_factor, const double* sg,
                                              const double* yb, double delta, double c03, double c04) {
  const int N = S.N, m = S.m, nb = S.nb;
  const double T = S.T;
  if (k > N) return;
  double Q[36];
#pragma unroll
  for (int t = 0; t < 36; ++t) Q[t] = 0.0;
  double s03 = 0.0, s04 = 0.0;
  if (k >= 1) {  // the stages whose state depends on w
    double Qxy0 = 0, Qxy1 = 0, Qxy2 = 0;
    double Qb[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < m; ++i) {
      const int r = k * m + i;
      const double w = (sg ? sg[r] : 0.0) + delta;
      if (i < nb) {
        Qb[i] = w;
      } else {
        const double C = yb ? yb[r] : 0.0;
        const ObsGeo d = obstacle_geo(S, k, i - nb);
        const double gx = -(d.ddx * d.idd), gy = -(d.ddy * d.idd);
        const ObsCurv h = obstacle_curvature(d, C);
        Qxy0 += w * gx * gx + h.h00;
        Qxy1 += w * gx * gy + h.h01;
        Qxy2 += w * gy * gy + h.h11;
      }
    }
    const int sv[6] = {0, 1, 2, 5, 6, 7};  // the states a stage cost reads
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int bq = a; bq < 6; ++bq) Q[S.pk8(sv[a], sv[bq])] += obj_factor * S.Hl[k * 21 + hp(a, bq)];
    }
    Q[S.pk8(0, 0)] += Qxy0; Q[S.pk8(0, 1)] += Qxy1; Q[S.pk8(1, 1)] += Qxy2;
    Q[S.pk8(2, 2)] += Qb[0]; Q[S.pk8(3, 3)] += Qb[1]; Q[S.pk8(5, 5)] += Qb[2];
    Q[S.pk8(6, 6)] += Qb[3]; Q[S.pk8(7, 7)] += Qb[4];
    if (k < N) {
      const Dyn2 e = point_dyn2(S, k);
      Q[S.pk8(3, 3)] += T * e.e33;
      Q[S.pk8(4, 4)] += T * e.e44;
      Q[S.pk8(3, 4)] += T * e.e34;
      s03 = T * e.e03;
      s04 = T * e.e04;
    }
  } else {
    s03 = c03;
    s04 = c04;
  }
#pragma unroll
  for (int t = 0; t < 36; ++t) S.Qs[k * 36 + t] = Q[t];
  LDS double* qo = S.qs + k * 10;
#pragma unroll
  for (int c = 0; c < 8; ++c) qo[c] = 0.0;
  qo[8] = s03;
  qo[9] = s04;
}

// lane k, 1 <= k <= N: q_k = G_k^T t over the stage's rows into the sweeps' LDS slots, t(i) the
// caller's value for row (k, i); without rows, zeros
template <class RowT>
__device__ __forceinline__ void point_stage_q(Solver<CapEv>& S, int k, bool rows, RowT t_of) {
  double q8[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) q8[c] = 0.0;
  if (rows) {
    double qx = 0.0, qy = 0.0;
    for (int i = 0; i < S.m; ++i) {
      const double t = t_of(i);
      if (i < S.nb) {
        const int bi = boxidx(i);
#pragma unroll
        for (int c = 2; c < 8; ++c) q8[c] = c == bi ? t : q8[c];
      } else {
        const ObsGeo d = obstacle_geo(S, k, i - S.nb);
        qx += t * (-(d.ddx * d.idd));
        qy += t * (-(d.ddy * d.idd));
      }
    }
    q8[0] = qx;
    q8[1] = qy;
  }
  LDS double* qo = S.qs + k * 10;
#pragma unroll
  for (int c = 0; c < 8; ++c) qo[c] = q8[c];
}

// which entries of a direction of p something reads (lane i: internal entry i), and the entry's
// place pe in the caller's layout.  An entry nothing reads is never loaded: a NaN there changes
// nothing
__device__ __forceinline__ bool point_reads(const Solver<CapEv>& S, const Params* __restrict__ prm, int lane, int& pe) {
  bool reads = lane < 10;
  if (lane == prm->w1p || lane == prm->w2p) reads = true;
  for (int o = 0; o < S.nobs; ++o)
    if (lane == prm->oxp[o] || lane == prm->oyp[o]) reads = true;
  pe = lane < prm->np ? ext_p(prm, lane) : -1;
  return reads && pe >= 0;
}

// ---- outputs, strided over the lanes

// a trajectory, 8 per stage in LDS, to the caller's nxE per stage
__device__ __forceinline__ void put_trajectory(const Params* __restrict__ prm, int lane, const LDS double* X8,
                                               double* o) {
  const int nxE = prm->nxE;
  for (int i = lane; i < prm->nX; i += WAVE) {
    const int kk = i >> 3, c = i & 7;
    if (c < nxE) o[kk * nxE + c] = X8[i];
  }
}
// rows (k, i) = G_{k,i} dX_k (Solver::row_jd); stage 0's are 0: it is constant in w
__device__ __forceinline__ void put_rows_jd(Solver<CapEv>& S, int lane, const LDS double* dX, double* o) {
  for (int r = lane; r < S.ng; r += WAVE) o[r] = r < S.m ? 0.0 : S.row_jd(r, dX);
}
// controls: B_k^T mu_{k+1} (Solver::grad_u) and, with `cross`, the cross term cr[k] = Hxu_k^T dX_k
// on the first control of every stage, stage 0's only with `stage0` (a w-direction's is absent)
__device__ __forceinline__ void put_grad_u(Solver<CapEv>& S, const Params* __restrict__ prm, int lane,
                                           const LDS double* cr, bool cross, bool stage0, double* o) {
  for (int i = lane; i < S.nw; i += WAVE) {
    const int e = ext_u(prm, i);
    if (e < 0) continue;
    const int kk = i / 6;
    const double g = S.grad_u(i);
    o[e] = (cross && i == 6 * kk && (stage0 || kk >= 1)) ? g + cr[kk] : g;
  }
}

}  // namespace
