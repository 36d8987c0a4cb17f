// nmpc_adjoint.hip -- batched adjoint (vector-Jacobian) products at GIVEN points
// (nmpc_adjoint_products_batch / nmpc_adjoint_products_batch_dev, include/nmpc_amd.h): for each
// of B scenarios and each of na seeds (y, z, Xb) on (g, grad_w L, X), with
// L = obj_factor f + lam_g' g and W = obj_factor grad^2 f + sum_i lam_g_i grad^2 g_i,
//   wbar = J_g' y + W z + (dX/dw)' Xb,   pbar = (dg/dp)' y + (d_p grad_w L)' z + (dX/dp)' Xb
// The transposed half of nmpc_products.hip and nmpc_pproducts.hip: one scalar loss on the
// function layer pulled back to all of w and all of p at the cost of one direction.
//
// Part of the evaluation kernel's translation unit (nmpc_eval.hip includes this file last), so
// the derivatives are the text the solver compiles: Solver::rollout, stage_cost,
// derivs<true, true>, adjoint, stage_AB, grad_u, and the curvature expressions of the two
// forward kernels.
//
// Execution model: the products kernels'.  One wavefront per (scenario, seed chunk), stage k on
// lane k, rows and variables strided over the lanes, control flow wave-uniform.
// Once per wavefront:
//   1. scenario data, rollout and stage costs as nmpc_products_kernel;
//   2. where a cost weight comes from p and a z seed will ask for it: the stage-cost gradients
//      with the weights (1, 0) and (0, 1), kept by lane k (as nmpc_pproducts_kernel);
//   3. derivs<true, true>: gl, Hl; adjoint(obj_factor, lam_g): lam_{k+1};
//   4. lane k keeps for every seed: obj_factor Hl_k (21 packed entries), the summed obstacle
//      curvature sum_o lam_{k,o} Hg_o, the dynamics terms d33, d34, d44, s03, s04 of
//      lam_{k+1}^T T f (k < N) and the entries of A_k = I + E_k and B_k's first column; each
//      obstacle's own lam_{k,o} Hg_o goes to the workspace where its centre comes from p.
// Per seed (reverse over forward; a NULL seed's terms are not formed):
//   5. z given: the forward tangent xi_0 = 0, xi_{k+1} = A_k xi_k + B_k z_k as in-order prefix
//      sums (nmpc_products_kernel's step 4), kept by lane k in registers;
//   6. the stage source s_k without its row part, into the gradient slice of the workspace:
//        Xb_k + obj_factor Hl_k xi_k + sum_o lam_{k,o} Hg_o xi_k + d2_xx(lam_{k+1}^T T f) xi_k
//             + Hxu_k z_k
//      (stage 0: xi_0 = 0 exactly, so only Xb_0 and Hxu_0 z_0; stage N: no dynamics follow it);
//   7. nu_k = s_k + G_k^T y_k + A_k^T nu_{k+1}: Solver::adjoint(1, y) -- stage 0's rows of y are
//      read, (dg/dp) has stage-0 rows;
//   8. wbar_{u_k} = B_k^T nu_{k+1} (Solver::grad_u) + Hxu_k^T xi_k (Huu = 0: the dynamics are
//      linear in the controls and no cost reads them);
//   9. pbar, lane i forming internal entry i: nu_0 at the x0 block; -sum_k (obj_factor Hl_k
//      xi_k)[0:2] at the target; -sum_k [y_{k,o} G_{k,o}[0:2] + lam_{k,o} (Hg_o xi_k)[0:2]] at an
//      obstacle centre taken from p; obj_factor sum_k gl_k^(1,0) . xi_k (resp. (0,1)) at a cost
//      weight taken from p; exactly 0 at an entry nothing reads.  The sums over stages are wave
//      reductions, as the solve's lam_p block.
// Every per-seed buffer is rewritten by each seed, so seeds are independent and the results do
// not depend on how they are dealt to wavefronts.
// (included by nmpc_eval.hip)

namespace {

static_assert(CapA::L.wstotal >= kAdjWs && CapB::L.wstotal >= kAdjWs && CapC::L.wstotal >= kAdjWs &&
                  CapD::L.wstotal >= kAdjWs && CapA32::L.wstotal >= kAdjWs && CapC32::L.wstotal >= kAdjWs &&
                  CapE::L.wstotal >= kAdjWs,
              "a solver class's workspace is smaller than one wavefront's of the adjoint-products kernel");

// LDS carve-up (doubles)
constexpr int R_PP = 0;                       // p, internal layout (<= 64)
constexpr int R_OB = R_PP + 64;               // obstacle x (16), y (16)
constexpr int R_RV = R_OB + 2 * NMPC_MAX_OBS; // Solver::rvars; [30], [31] = cost weights
constexpr int R_ST = R_RV + 32;               // phase-timer slots (NMPC_STAMPS builds write them)
constexpr int R_X = R_ST + PH_COUNT;          // trajectory, 8 per stage
constexpr int R_TRIG = R_X + 8 * NS;
constexpr int R_INC = R_TRIG + 8 * NS;        // prefix / suffix sum scratch
constexpr int R_LAM = R_INC + 8 * NS;         // lam, then each seed's nu
constexpr int R_CR = R_LAM + 8 * NS;          // the seed's Hxu_k^T xi_k
constexpr int R_TOTAL = R_CR + NS;
static_assert(R_TOTAL * 8 <= 32 * 1024, "adjoint-products kernel LDS");

__global__ __launch_bounds__(WAVE) void nmpc_adjoint_kernel(const Params* __restrict__ prm, int B, int chunks,
                                                            AdjIO io) {
  __shared__ __attribute__((aligned(16))) double smem[R_TOTAL];
  const int b = blockIdx.x, chunk = blockIdx.y;
  if (b >= B) return;
  Solver<CapEv> S{};
  LDS double* sm = (LDS double*)smem;
  GLB double* gw = (GLB double*)(io.ws + ((long long)b * chunks + chunk) * kAdjWs);
  S.P = (const CST Params*)prm; S.sm = sm; S.lane_ = threadIdx.x; S.b = b;
  S.N = prm->N; S.m = prm->m; S.nobs = prm->nobs; S.nw = prm->nw; S.ng = prm->ng; S.T = prm->T;
  S.nb = prm->nb; S.nuE = prm->nuE; S.nwE = prm->nwE;
  S.U = gw + kProdU; S.gl = gw + kProdGl; S.Hl = gw + kProdHl; S.tc = gw + kProdTc; S.dc = gw + kProdDc;
  S.pp = sm + R_PP; S.obx = sm + R_OB; S.oby = S.obx + NMPC_MAX_OBS; S.rvars = sm + R_RV; S.stamps = sm + R_ST;
  S.X = sm + R_X; S.trig = sm + R_TRIG; S.inc = sm + R_INC; S.lam = sm + R_LAM;
  GLB double* oc = gw + kPprodOc;
  LDS double* cr = sm + R_CR;
  const int N = S.N, m = S.m, nb = S.nb, nw = S.nw, ng = S.ng, nwE = S.nwE, np = prm->np, npE = prm->npE;
  const int nxE = prm->nxE, nXE = nxE * (N + 1);
  const int w1p = prm->w1p, w2p = prm->w2p;
  const double sig = io.obj_factor;
  const double T = S.T;
  const int lane = S.lanef();
  const double* yb = io.lam_g ? io.lam_g + (long long)b * io.ld_lam_g : nullptr;
  const double* xb = io.x + (long long)b * io.ld_x;
  const double* ys = io.y ? io.y + (long long)b * io.ld_y : nullptr;
  const double* zs = io.z ? io.z + (long long)b * io.ld_z : nullptr;
  const double* Xs = io.Xb ? io.Xb + (long long)b * io.ld_Xb : nullptr;
  const bool zp = zs && io.pbar;  // the p-side terms of a z seed are asked for

  // ---------------- scenario data (as nmpc_products_kernel loads it)
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

  // ---------------- cost weights from p: unit-weight gradients, lane k stage k's
  double g10[6], g01[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) g10[a] = g01[a] = 0.0;
  if (zp && (w1p >= 0 || w2p >= 0)) {
    const double w1s = S.rvars[30], w2s = S.rvars[31];
    sync();
    if (w1p >= 0) {
      if (lane == 0) { S.rvars[30] = 1.0; S.rvars[31] = 0.0; }
      sync();
      S.derivs<false, true>(S.X, S.U, S.tc);
      if (k < N) {
#pragma unroll
        for (int a = 0; a < 6; ++a) g10[a] = S.gl[k * 8 + sv[a]];
      }
    }
    if (w2p >= 0) {
      if (lane == 0) { S.rvars[30] = 0.0; S.rvars[31] = 1.0; }
      sync();
      S.derivs<false, true>(S.X, S.U, S.tc);
      if (k < N) {
#pragma unroll
        for (int a = 0; a < 6; ++a) g01[a] = S.gl[k * 8 + sv[a]];
      }
    }
    if (lane == 0) { S.rvars[30] = w1s; S.rvars[31] = w2s; }
    sync();
  }

  // ---------------- derivatives and multipliers at the scenario's own weights
  S.derivs<true, true>(S.X, S.U, S.tc);
  if (yb) S.adjoint(sig, yb);
  else S.adjoint(sig, (const double*)nullptr);

  // ---------------- lane k: stage k's second-order data, kept in registers
  double Hc[21];
#pragma unroll
  for (int t = 0; t < 21; ++t) Hc[t] = 0.0;
  double q00 = 0.0, q01 = 0.0, q11 = 0.0;
  double d33 = 0.0, d34 = 0.0, d44 = 0.0, s03 = 0.0, s04 = 0.0;
  double E03 = 0.0, E04 = 0.0, E13 = 0.0, E14 = 0.0, E23 = 0.0, b00 = 0.0, b10 = 0.0, b20 = 0.0;
  if (k < N) S.stage_AB(k, E03, E04, E13, E14, E23, b00, b10, b20);
  if (zs) {
    if (stage) {
#pragma unroll
      for (int t = 0; t < 21; ++t) Hc[t] = sig * S.Hl[k * 21 + t];
      if (yb) {  // y-weighted obstacle curvature: nmpc_products_kernel's, rows in order
        const LDS double* xk = S.X + k * 8;
        for (int o = 0; o < S.nobs; ++o) {
          const double C = yb[k * m + nb + o];
          const double ddx = xk[0] - S.obx[o], ddy = xk[1] - S.oby[o];
          const double idd = rsq(ddx * ddx + ddy * ddy);
          const double id3 = idd * idd * idd;
          const double h00 = C * (-ddy * ddy * id3), h01 = C * (ddx * ddy * id3), h11 = C * (-ddx * ddx * id3);
          q00 += h00; q01 += h01; q11 += h11;
          if (io.pbar && (prm->oxp[o] >= 0 || prm->oyp[o] >= 0)) {
            GLB double* q = oc + (k * NMPC_MAX_OBS + o) * 3;
            q[0] = h00; q[1] = h01; q[2] = h11;
          }
        }
      }
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
  // the internal entry of p this lane forms, and its place in the caller's layout
  const int pe = lane < np ? ext_p(prm, lane) : -1;
  sync();  // lam is rewritten by every seed's sweep

  // ---------------- seeds c, c + chunks, ...
  for (int d = chunk; d < io.na; d += chunks) {
    const double* yd = ys ? ys + (long long)d * ng : nullptr;
    const double* zd = zs ? zs + (long long)d * nwE : nullptr;
    const double* Xd = Xs ? Xs + (long long)d * nXE : nullptr;
    double dx[8], du0 = 0.0;
#pragma unroll
    for (int c = 0; c < 8; ++c) dx[c] = 0.0;
    // 5. forward tangent of the z seed
    if (zd) {
      double du[6];
#pragma unroll
      for (int c = 0; c < 6; ++c) du[c] = (k < N && c < S.nuE) ? zd[k * S.nuE + c] : 0.0;
      du0 = du[0];
      if (k < N) {
#pragma unroll
        for (int c = 0; c < 5; ++c) S.inc[k * 8 + c] = T * du[1 + c];
      }
      sync();
      if (k <= N) {
        for (int j = 0; j < k; ++j) {
#pragma unroll
          for (int c = 0; c < 5; ++c) dx[3 + c] = dx[3 + c] + S.inc[j * 8 + c];
        }
        if (k < N) {  // stage 0: xi_0 = 0, only B_0 z_0
          S.inc[k * 8 + 5] = k == 0 ? b00 * du0 : (E03 * dx[3] + E04 * dx[4]) + b00 * du0;
          S.inc[k * 8 + 6] = k == 0 ? b10 * du0 : (E13 * dx[3] + E14 * dx[4]) + b10 * du0;
          S.inc[k * 8 + 7] = k == 0 ? b20 * du0 : E23 * dx[3] + b20 * du0;
        }
      }
      sync();
      if (k <= N) {
        for (int j = 0; j < k; ++j) {
          dx[0] = dx[0] + S.inc[j * 8 + 5];
          dx[1] = dx[1] + S.inc[j * 8 + 6];
          dx[2] = dx[2] + S.inc[j * 8 + 7];
        }
      }
    }
    // 6. the stage source without its rows, and the cross term of step 8
    double t0 = 0.0, t1 = 0.0;  // (obj_factor Hl_k xi_k)[0:2]: the target's part of pbar
    if (k <= N) {
      double hs[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) hs[c] = 0.0;
      if (zd) {
        if (stage) {
#pragma unroll
          for (int a = 0; a < 6; ++a) {
            double acc = 0.0;
#pragma unroll
            for (int q = 0; q < 6; ++q) acc += Hc[hp(a, q)] * dx[sv[q]];
            hs[sv[a]] = acc;
          }
          if (k < N) { t0 = hs[0]; t1 = hs[1]; }
          if (yb && S.nobs > 0) {
            hs[0] += q00 * dx[0] + q01 * dx[1];
            hs[1] += q01 * dx[0] + q11 * dx[1];
          }
          // (stage N: no dynamics follow it, its terms are absent)
          hs[3] = k < N ? (d33 * dx[3] + d34 * dx[4]) + s03 * du0 : 0.0;
          hs[4] = k < N ? (d34 * dx[3] + d44 * dx[4]) + s04 * du0 : 0.0;
          cr[k] = k < N ? s03 * dx[3] + s04 * dx[4] : 0.0;
        } else {  // stage 0: Hxu_0 z_0 alone
          hs[3] = k < N ? s03 * du0 : 0.0;
          hs[4] = k < N ? s04 * du0 : 0.0;
          cr[k] = 0.0;
        }
      }
      GLB double* h = S.gl + k * 8;
      if (Xd) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          if (c < nxE) {
            const double xv = Xd[k * nxE + c];
            hs[c] = zd ? hs[c] + xv : xv;
          }
        }
      }
#pragma unroll
      for (int c = 0; c < 8; ++c) h[c] = hs[c];
    }
    sync();
    // 7. nu_k = s_k + G_k^T y_k + A_k^T nu_{k+1}
    if (yd) S.adjoint(1.0, yd);
    else S.adjoint(1.0, (const double*)nullptr);
    // 8. wbar
    if (io.wbar) {
      double* o = io.wbar + ((long long)b * io.na + d) * nwE;
      for (int i = lane; i < nw; i += WAVE) {
        const int e = ext_u(prm, i);
        if (e < 0) continue;
        const int kk = i / 6;
        const double g = S.grad_u(i);
        o[e] = (zd && i == 6 * kk && kk >= 1) ? g + cr[kk] : g;
      }
    }
    // 9. pbar
    if (io.pbar) {
      double v = lane < 8 ? S.lam[lane] : 0.0;
      if (zd) {
        const double gxt = -wsum(t0);
        const double gyt = -wsum(t1);
        if (lane == 8) v = gxt;
        else if (lane == 9) v = gyt;
        if (w1p >= 0) {
          double a_ = 0.0;
#pragma unroll
          for (int a = 0; a < 6; ++a) a_ += g10[a] * dx[sv[a]];
          const double s = sig * wsum(stage ? a_ : 0.0);
          if (lane == w1p) v += s;
        }
        if (w2p >= 0) {
          double a_ = 0.0;
#pragma unroll
          for (int a = 0; a < 6; ++a) a_ += g01[a] * dx[sv[a]];
          const double s = sig * wsum(stage ? a_ : 0.0);
          if (lane == w2p) v += s;
        }
      }
      if (yd || (zd && yb)) {
        for (int o = 0; o < S.nobs; ++o) {
          const int ix = prm->oxp[o], iy = prm->oyp[o];
          if (ix < 0 && iy < 0) continue;
          double cx = 0.0, cy = 0.0;
          if (k <= N) {
            if (yd) {  // row g = r_sum - |(x, y) - (ox, oy)|: dg/dox = (x - ox) / d
              const double yv = yd[k * m + nb + o];
              const LDS double* xk = S.X + k * 8;
              const double ddx = xk[0] - S.obx[o], ddy = xk[1] - S.oby[o];
              const double idd = rsq(ddx * ddx + ddy * ddy);
              cx = yv * (ddx * idd);
              cy = yv * (ddy * idd);
            }
            if (zd && yb && stage) {  // the centre's move against the obstacle's own curvature
              const GLB double* q = oc + (k * NMPC_MAX_OBS + o) * 3;
              cx -= q[0] * dx[0] + q[1] * dx[1];
              cy -= q[1] * dx[0] + q[2] * dx[1];
            }
          }
          cx = wsum(cx); cy = wsum(cy);
          if (lane == ix) v += cx;
          if (lane == iy) v += cy;
        }
      }
      if (pe >= 0) io.pbar[((long long)b * io.na + d) * npE + pe] = v;
    }
    sync();
  }
}

}  // namespace

int nmpc_adjoint_launch(const Params* dprm, int B, int chunks, const AdjIO& io, void* stream) {
  hipLaunchKernelGGL(nmpc_adjoint_kernel, dim3(B, chunks), dim3(WAVE), 0, (hipStream_t)stream, dprm, B, chunks, io);
  return (int)hipGetLastError();
}
