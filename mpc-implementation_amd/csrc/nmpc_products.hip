// nmpc_products.hip -- batched Jacobian- and Hessian-vector products at GIVEN points
// (nmpc_products_batch / nmpc_products_batch_dev, include/nmpc_amd.h): for each of B
// scenarios and each of nv directions v in decision space
//   J_g(x, p) v,   (obj_factor grad^2 f + sum_i lam_g_i grad^2 g_i) v,   (dX/dw) v
// CasADi's nlp_jac_g and nlp_hess_l applied to a vector; oracle SSEval.J, SSEval.hessian
// and SSEval.Z without forming Z.
//
// Part of the evaluation kernel's translation unit: nmpc_eval.hip includes this file after
// its own kernel, so the solver's source is seen with no class selected and the second
// derivatives here are the text the solver compiles -- Solver::derivs<true> (Hl),
// Solver::adjoint (the dynamics multipliers, and again for the sweep over h), the obstacle
// curvature and the five dynamics terms of Solver::assemble, Solver::row_jd, Solver::grad_u.
//
// Execution model: the solver's.  One wavefront per (scenario, direction chunk), stage k on
// lane k, rows and decision variables strided over the lanes, control flow wave-uniform.
// Once per wavefront:
//   1. scenario data, rollout and stage costs as nmpc_eval_kernel (the stage costs fill the
//      transcendental cache that derivs<true, true> reads);
//   2. derivs<true, true>: gl, Hl; adjoint(obj_factor, lam_g): lam_{k+1};
//   3. lane k keeps its stage's second-order data in registers for every direction:
//      Hq = obj_factor Hl_k + sum_o lam_{k,o} Hg_o (21 packed entries over x, y, z, x5, x6, x7),
//      the dynamics terms d33, d34, d44 (theta, psi) and s03, s04 (theta / psi against v) of
//      lam_{k+1}^T T f (k < N), and the entries of A_k = I + E_k and of B_k's first column.
// Per direction (forward over reverse):
//   4. tangent rollout dX_0 = 0, dX_{k+1} = A_k dX_k + B_k du_k as in-order prefix sums, the
//      angles first and then the positions, as Solver::rollout;
//   5. J v: row (k, i) = G_{k,i} dX_k (Solver::row_jd), rows strided over the lanes;
//   6. h_k = Hxx_k dX_k + Hxu_k du_k (k >= 1) into the gradient slice of the workspace;
//   7. mu_k = h_k + A_k^T mu_{k+1}: Solver::adjoint(1, no rows) on that slice;
//   8. (W v)_{u_k} = B_k^T mu_{k+1} (Solver::grad_u) + Hxu_k^T dX_k.
// Stage 0 is constant in w: dX_0 and its rows are written as 0 and its terms are never
// formed (no 0 * NaN).  Every per-direction buffer is rewritten by each direction, and a
// lane's sums take only the stages its result depends on, so directions are independent and
// the results do not depend on how the directions are dealt to wavefronts.
// (included by nmpc_eval.hip)

namespace {

static_assert(CapA::L.wstotal >= kProdWs && CapB::L.wstotal >= kProdWs && CapC::L.wstotal >= kProdWs &&
                  CapD::L.wstotal >= kProdWs && CapA32::L.wstotal >= kProdWs && CapC32::L.wstotal >= kProdWs &&
                  CapE::L.wstotal >= kProdWs,
              "a solver class's workspace is smaller than one wavefront's of the products kernel");

// LDS carve-up (doubles)
constexpr int P_PP = 0;                       // p, internal layout (<= 64)
constexpr int P_OB = P_PP + 64;               // obstacle x (16), y (16)
constexpr int P_RV = P_OB + 2 * NMPC_MAX_OBS; // Solver::rvars; [30], [31] = cost weights
constexpr int P_ST = P_RV + 32;               // phase-timer slots (NMPC_STAMPS builds write them)
constexpr int P_X = P_ST + PH_COUNT;          // trajectory, 8 per stage
constexpr int P_TRIG = P_X + 8 * NS;
constexpr int P_INC = P_TRIG + 8 * NS;        // prefix / suffix sum scratch
constexpr int P_LAM = P_INC + 8 * NS;         // lam, then each direction's mu
constexpr int P_DX = P_LAM + 8 * NS;          // the direction's tangent trajectory
constexpr int P_CR = P_DX + 8 * NS;           // the direction's Hxu_k^T dX_k
constexpr int P_TOTAL = P_CR + NS;
static_assert(P_TOTAL * 8 <= 32 * 1024, "products kernel LDS");

__global__ __launch_bounds__(WAVE) void nmpc_products_kernel(const Params* __restrict__ prm, int B, int chunks,
                                                             ProdIO io) {
  __shared__ __attribute__((aligned(16))) double smem[P_TOTAL];
  const int b = blockIdx.x, chunk = blockIdx.y;
  if (b >= B) return;
  Solver<CapEv> S{};
  LDS double* sm = (LDS double*)smem;
  GLB double* gw = (GLB double*)(io.ws + ((long long)b * chunks + chunk) * kProdWs);
  S.P = (const CST Params*)prm; S.sm = sm; S.lane_ = threadIdx.x; S.b = b;
  S.N = prm->N; S.m = prm->m; S.nobs = prm->nobs; S.nw = prm->nw; S.ng = prm->ng; S.T = prm->T;
  S.nb = prm->nb; S.nuE = prm->nuE; S.nwE = prm->nwE;
  S.U = gw + kProdU; S.gl = gw + kProdGl; S.Hl = gw + kProdHl; S.tc = gw + kProdTc; S.dc = gw + kProdDc;
  S.pp = sm + P_PP; S.obx = sm + P_OB; S.oby = S.obx + NMPC_MAX_OBS; S.rvars = sm + P_RV; S.stamps = sm + P_ST;
  S.X = sm + P_X; S.trig = sm + P_TRIG; S.inc = sm + P_INC; S.lam = sm + P_LAM;
  LDS double* dX = sm + P_DX;
  LDS double* cr = sm + P_CR;
  const int N = S.N, m = S.m, nb = S.nb, nw = S.nw, ng = S.ng, nwE = S.nwE;
  const int nxE = prm->nxE, nXE = nxE * (N + 1);
  const double T = S.T;
  const int lane = S.lanef();
  const double* yb = io.lam_g ? io.lam_g + (long long)b * io.ld_lam_g : nullptr;
  const double* xb = io.x + (long long)b * io.ld_x;
  const double* vb = io.v + (long long)b * io.ld_v;

  // ---------------- scenario data (as nmpc_eval_kernel loads it)
  if (lane < PH_COUNT) S.stamps[lane] = 0.0;
  for (int i = lane; i < prm->np; i += WAVE) {
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
    S.rvars[30] = prm->w1p >= 0 ? S.pp[prm->w1p] : prm->w1;
    S.rvars[31] = prm->w2p >= 0 ? S.pp[prm->w2p] : prm->w2;
  }
  for (int i = lane; i < nw; i += WAVE) {
    const int e = ext_u(prm, i);
    S.U[i] = e >= 0 ? xb[e] : 0.0;
  }
  for (int r = lane; r < ng; r += WAVE) S.dc[r] = 1.0;  // unscaled rows
  sync();

  // ---------------- rollout, stage costs (their transcendentals), derivatives, multipliers
  S.rollout(S.U, S.X);
  if (lane < N) (void)S.stage_cost(S.X + lane * 8, S.tc + lane * 12);
  sync();
  S.derivs<true, true>(S.X, S.U, S.tc);
  if (yb) S.adjoint(io.obj_factor, yb);
  else S.adjoint(io.obj_factor, (const double*)nullptr);

  // ---------------- lane k: stage k's second-order data, kept in registers
  const int k = lane;
  const bool stage = k >= 1 && k <= N;  // the stages whose state depends on w
  double Hq[21];
#pragma unroll
  for (int t = 0; t < 21; ++t) Hq[t] = 0.0;
  double d33 = 0.0, d34 = 0.0, d44 = 0.0, s03 = 0.0, s04 = 0.0;
  double E03 = 0.0, E04 = 0.0, E13 = 0.0, E14 = 0.0, E23 = 0.0, b00 = 0.0, b10 = 0.0, b20 = 0.0;
  if (k < N) S.stage_AB(k, E03, E04, E13, E14, E23, b00, b10, b20);
  if (stage) {
#pragma unroll
    for (int t = 0; t < 21; ++t) Hq[t] = io.obj_factor * S.Hl[k * 21 + t];
    if (yb) {  // y-weighted obstacle curvature: Solver::assemble's, rows in order
      const LDS double* xk = S.X + k * 8;
      double q00 = 0.0, q01 = 0.0, q11 = 0.0;
      for (int o = 0; o < S.nobs; ++o) {
        const double C = yb[k * m + nb + o];
        const double ddx = xk[0] - S.obx[o], ddy = xk[1] - S.oby[o];
        const double idd = rsq(ddx * ddx + ddy * ddy);
        const double id3 = idd * idd * idd;
        q00 += C * (-ddy * ddy * id3);
        q01 += C * (ddx * ddy * id3);
        q11 += C * (-ddx * ddx * id3);
      }
      if (S.nobs > 0) { Hq[hp(0, 0)] += q00; Hq[hp(0, 1)] += q01; Hq[hp(1, 1)] += q11; }
    }
    if (k < N) {  // second derivatives of lam_{k+1}^T T f(x_k, u_k): Solver::assemble's dyn branch
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
  }
  sync();  // lam is rewritten by every direction's sweep

  // ---------------- directions c, c + chunks, ...
  for (int d = chunk; d < io.nv; d += chunks) {
    const double* vd = vb + (long long)d * nwE;
    // 4. tangent rollout
    double du[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) du[c] = (k < N && c < S.nuE) ? vd[k * S.nuE + c] : 0.0;
    if (k < N) {
#pragma unroll
      for (int c = 0; c < 5; ++c) S.inc[k * 8 + c] = T * du[1 + c];
    }
    sync();
    double dx[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) dx[c] = 0.0;
    if (k <= N) {
      for (int j = 0; j < k; ++j) {
#pragma unroll
        for (int c = 0; c < 5; ++c) dx[3 + c] = dx[3 + c] + S.inc[j * 8 + c];
      }
      if (k < N) {  // stage 0: dX_0 = 0, only B_0 du_0
        S.inc[k * 8 + 5] = k == 0 ? b00 * du[0] : (E03 * dx[3] + E04 * dx[4]) + b00 * du[0];
        S.inc[k * 8 + 6] = k == 0 ? b10 * du[0] : (E13 * dx[3] + E14 * dx[4]) + b10 * du[0];
        S.inc[k * 8 + 7] = k == 0 ? b20 * du[0] : E23 * dx[3] + b20 * du[0];
      }
    }
    sync();
    if (k <= N) {
      for (int j = 0; j < k; ++j) {
        dx[0] = dx[0] + S.inc[j * 8 + 5];
        dx[1] = dx[1] + S.inc[j * 8 + 6];
        dx[2] = dx[2] + S.inc[j * 8 + 7];
      }
#pragma unroll
      for (int c = 0; c < 8; ++c) dX[k * 8 + c] = dx[c];
    }
    // 6. h_k, and the cross term of step 8
    if (k <= N) {
      GLB double* h = S.gl + k * 8;
      if (stage) {
        const int sv[6] = {0, 1, 2, 5, 6, 7};
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          double acc = 0.0;
#pragma unroll
          for (int q = 0; q < 6; ++q) acc += Hq[hp(a, q)] * dx[sv[q]];
          h[sv[a]] = acc;
        }
        // (stage N: no dynamics follow it, its terms are absent)
        h[3] = k < N ? (d33 * dx[3] + d34 * dx[4]) + s03 * du[0] : 0.0;
        h[4] = k < N ? (d34 * dx[3] + d44 * dx[4]) + s04 * du[0] : 0.0;
        cr[k] = k < N ? s03 * dx[3] + s04 * dx[4] : 0.0;
      } else {
#pragma unroll
        for (int c = 0; c < 8; ++c) h[c] = 0.0;
        cr[k] = 0.0;
      }
    }
    sync();
    // 5. J v and the tangent out
    if (io.jv) {
      double* o = io.jv + ((long long)b * io.nv + d) * ng;
      for (int r = lane; r < ng; r += WAVE) o[r] = r < m ? 0.0 : S.row_jd(r, dX);
    }
    if (io.dX) {
      double* o = io.dX + ((long long)b * io.nv + d) * nXE;
      for (int i = lane; i < prm->nX; i += WAVE) {
        const int kk = i >> 3, c = i & 7;
        if (c < nxE) o[kk * nxE + c] = dX[i];
      }
    }
    if (!io.hv) {
      sync();
      continue;
    }
    // 7. mu_k = h_k + A_k^T mu_{k+1}
    S.adjoint(1.0, (const double*)nullptr);
    // 8. (W v)_{u_k}
    double* o = io.hv + ((long long)b * io.nv + d) * nwE;
    for (int i = lane; i < nw; i += WAVE) {
      const int e = ext_u(prm, i);
      if (e < 0) continue;
      const int kk = i / 6;
      const double g = S.grad_u(i);
      o[e] = (i == 6 * kk && kk >= 1) ? g + cr[kk] : g;
    }
    sync();
  }
}

}  // namespace

int nmpc_products_launch(const Params* dprm, int B, int chunks, const ProdIO& io, void* stream) {
  hipLaunchKernelGGL(nmpc_products_kernel, dim3(B, chunks), dim3(WAVE), 0, (hipStream_t)stream, dprm, B, chunks, io);
  return (int)hipGetLastError();
}
