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
//   1. scenario data, rollout and stage costs (load_params, load_controls, point_rollout of
//      nmpc_eval_shared.hip);
//   2. where a cost weight comes from p and a z seed will ask for it: the stage-cost gradients
//      with the weights (1, 0) and (0, 1), kept by lane k (unit_weight_grads);
//   3. derivs<true, true>: gl, Hl; adjoint(obj_factor, lam_g): lam_{k+1};
//   4. lane k keeps for every seed: obj_factor Hl_k (21 packed entries), the summed obstacle
//      curvature sum_o lam_{k,o} Hg_o, the dynamics terms d33, d34, d44, s03, s04 of
//      lam_{k+1}^T T f (k < N) and the entries of A_k = I + E_k and B_k's first column; each
//      obstacle's own lam_{k,o} Hg_o goes to the workspace where its centre comes from p.
// Per seed (reverse over forward; a NULL seed's terms are not formed):
//   5. z given: the forward tangent xi_0 = 0, xi_{k+1} = A_k xi_k + B_k z_k as in-order prefix
//      sums (nmpc_products_kernel's step 4: a copy), kept by lane k in registers;
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

static_assert(fits_every_class(kAdjWs),
              "a solver class's workspace is smaller than one wavefront's of the adjoint-products kernel");

// LDS carve-up (doubles): the unit's head (its multipliers' buffer holds lam, then each seed's
// nu), then
constexpr int R_CR = B_END;                   // the seed's Hxu_k^T xi_k
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
  bind_solver(S, prm, sm, gw, b, kProdU, kProdGl, kProdHl, kProdTc, kProdDc);
  GLB double* oc = gw + kPprodOc;
  LDS double* cr = sm + R_CR;
  const int N = S.N, m = S.m, nb = S.nb, ng = S.ng, nwE = S.nwE, np = prm->np, npE = prm->npE;
  const int nxE = prm->nxE, nXE = nxE * (N + 1);
  const int w1p = prm->w1p, w2p = prm->w2p;
  const double sig = io.obj_factor;
  const double T = S.T;
  const int lane = S.lanef();
  const double* yb = io.lam_g ? io.lam_g + (long long)b * io.ld_lam_g : nullptr;
  const double* ys = io.y ? io.y + (long long)b * io.ld_y : nullptr;
  const double* zs = io.z ? io.z + (long long)b * io.ld_z : nullptr;
  const double* Xs = io.Xb ? io.Xb + (long long)b * io.ld_Xb : nullptr;
  const bool zp = zs && io.pbar;  // the p-side terms of a z seed are asked for

  // ---------------- scenario data, rollout and stage costs
  load_params(S, prm, lane, io.p + (long long)b * io.ld_p);
  load_controls(S, prm, lane, io.x + (long long)b * io.ld_x, true);
  sync();
  point_rollout(S, lane);

  const int k = lane;
  const bool stage = k >= 1 && k <= N;  // the stages whose state depends on w
  const int sv[6] = {0, 1, 2, 5, 6, 7};  // the states a stage cost reads

  // ---------------- cost weights from p: unit-weight gradients ((1, 0): gu[0:6], (0, 1):
  // gu[6:12]), lane k stage k's
  double gu[12];
#pragma unroll
  for (int a = 0; a < 12; ++a) gu[a] = 0.0;
  if (zp) unit_weight_grads(S, prm, lane, [&](int s, double g) { gu[s] = g; });

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
  const StageAB ab = point_stage_ab(S, k);
  if (zs) {
    if (stage) {
#pragma unroll
      for (int t = 0; t < 21; ++t) Hc[t] = sig * S.Hl[k * 21 + t];
      if (yb) {  // y-weighted obstacle curvature, rows in order, over the stages k >= 1 alone
        for (int o = 0; o < S.nobs; ++o) {
          const ObsCurv h = obstacle_curvature(S, k, o, yb[k * m + nb + o]);
          q00 += h.h00; q01 += h.h01; q11 += h.h11;
          if (io.pbar && (prm->oxp[o] >= 0 || prm->oyp[o] >= 0)) {
            GLB double* q = oc + (k * NMPC_MAX_OBS + o) * 3;
            q[0] = h.h00; q[1] = h.h01; q[2] = h.h11;
          }
        }
      }
    }
    if (k < N) {
      const Dyn2 e = point_dyn2(S, k);
      d33 = T * e.e33; d44 = T * e.e44; d34 = T * e.e34;
      s03 = T * e.e03; s04 = T * e.e04;
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
          S.inc[k * 8 + 5] = k == 0 ? ab.b00 * du0 : (ab.E03 * dx[3] + ab.E04 * dx[4]) + ab.b00 * du0;
          S.inc[k * 8 + 6] = k == 0 ? ab.b10 * du0 : (ab.E13 * dx[3] + ab.E14 * dx[4]) + ab.b10 * du0;
          S.inc[k * 8 + 7] = k == 0 ? ab.b20 * du0 : ab.E23 * dx[3] + ab.b20 * du0;
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
    if (io.wbar) put_grad_u(S, prm, lane, cr, zd != nullptr, false, io.wbar + ((long long)b * io.na + d) * nwE);
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
          for (int a = 0; a < 6; ++a) a_ += gu[a] * dx[sv[a]];
          const double s = sig * wsum(stage ? a_ : 0.0);
          if (lane == w1p) v += s;
        }
        if (w2p >= 0) {
          double a_ = 0.0;
#pragma unroll
          for (int a = 0; a < 6; ++a) a_ += gu[6 + a] * dx[sv[a]];
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
