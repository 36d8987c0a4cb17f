// nmpc_pproducts.hip -- batched parameter-direction products at GIVEN points
// (nmpc_param_products_batch / nmpc_param_products_batch_dev, include/nmpc_amd.h): for each of
// B scenarios and each of nd directions dp in parameter space, with L = obj_factor f + lam_g' g,
//   (dg/dp) dp,   (d_p grad_w L) dp,   (dX/dp) dp
// and, independent of the directions, grad_p L.  The parameter half of nmpc_products.hip: what
// changes from one MPC step to the next -- the initial state, the target, obstacle centres and
// cost weights taken from p -- differentiated exactly, at any point.
//
// Part of the evaluation kernel's translation unit like nmpc_products.hip (nmpc_eval.hip
// includes this file after nmpc_kkt.hip), so the derivatives are the text the solver compiles:
// Solver::rollout, stage_cost, derivs<true, true>, adjoint, stage_AB, row_jd, grad_u.
//
// Execution model: the products kernel's.  One wavefront per (scenario, direction chunk),
// stage k on lane k, rows and variables strided over the lanes, control flow wave-uniform.
// Once per wavefront:
//   1. scenario data, rollout and stage costs.  This kernel takes the unit's LDS head and
//      bind_solver from nmpc_eval_shared.hip and keeps its own text for everything else: each
//      helper tried in its place changed the kernel's instructions, and the kernel with them
//      measured slower;
//   2. where a cost weight comes from p: the stage costs and their gradients with the weights
//      (1, 0) and (0, 1) (stage_cost and derivs<false, true> on the swapped weights, as the
//      solve's lam_p block forms the unit-weight costs), kept by lane k;
//   3. derivs<true, true>: gl, Hl; adjoint(obj_factor, lam_g): lam_k for k = 0 .. N -- lam_0,
//      which no w-side kernel reads, is grad_p L's x0 block;
//   4. lane k keeps for every direction: obj_factor Hl_k (21 packed entries), the summed
//      obstacle curvature sum_o lam_{k,o} Hg_o, the dynamics terms d33, d34, d44, s03, s04 of
//      lam_{k+1}^T T f (k < N), the entries of A_k = I + E_k and the unit-weight gradients;
//      each obstacle's own lam_{k,o} Hg_o goes to the workspace (read back by the same lane);
//   5. wavefront (b, 0): grad_p L -- lam_0; -obj_factor sum_k gl_k[0:2] at the target;
//      -sum_k lam_{k,o} G_{k,o}[0:2] at an obstacle centre; obj_factor sum_k of the unit-weight
//      costs at a weight; exactly 0 at an entry nothing reads.
// Per direction (forward over reverse):
//   6. the entries of dp that something reads, to LDS in the kernel's p layout (an entry
//      nothing reads is never loaded: a NaN there changes nothing);
//   7. state tangent xi_0 = dp[0:nx], xi_{k+1} = A_k xi_k: the angles are constant over the
//      stages (no control term), the positions in-order prefix sums as Solver::rollout;
//   8. h_k for k = 0 .. N.  The stage cost reads the target only through (x - xt, y - yt) and
//      an obstacle row its centre only through (x - ox, y - oy), so a move of either acts like
//      the opposite move of the state, seen by that term alone:
//        h_k = obj_factor Hl_k (xi_k - target move) + sum_o lam_{k,o} Hg_o (xi_k - move_o)
//              + d2_xx(lam_{k+1}^T T f) xi_k + obj_factor (dw1 gl_k^(1,0) + dw2 gl_k^(0,1));
//   9. (dg/dp) dp: row (k, i) = G_{k,i} (xi_k - move_i) by Solver::row_jd, lane k forming its
//      stage's rows on a copy of xi_k moved for that row;
//  10. mu_k = h_k + A_k^T mu_{k+1}: Solver::adjoint(1, no rows) on the gradient slice;
//  11. (d_p grad_w L dp)_{u_k} = B_k^T mu_{k+1} (Solver::grad_u) + Hxu_k^T xi_k, k = 0 .. N - 1.
// Unlike the w-side products stage 0 is not constant: xi_0 = dp[0:nx] and B_0 depends on
// theta_0, psi_0.  A term that does not exist (a constant obstacle's move, a constant weight's
// tangent) is not formed, rather than multiplied by 0.  Every per-direction buffer is rewritten
// by each direction, so directions are independent and the results do not depend on how they
// are dealt to wavefronts.
// (included by nmpc_eval.hip)

namespace {

static_assert(fits_every_class(kPprodWs),
              "a solver class's workspace is smaller than one wavefront's of the parameter-products kernel");

// LDS carve-up (doubles): the unit's head (its multipliers' buffer holds lam, then each
// direction's mu), then
constexpr int Q_DX = B_END;                   // the direction's state tangent xi
constexpr int Q_CR = Q_DX + 8 * NS;           // the direction's Hxu_k^T xi_k
constexpr int Q_DP = Q_CR + NS;               // the direction, internal p layout (<= 64)
constexpr int Q_TOTAL = Q_DP + 64;
static_assert(Q_TOTAL * 8 <= 32 * 1024, "parameter-products kernel LDS");

__global__ __launch_bounds__(WAVE) void nmpc_pproducts_kernel(const Params* __restrict__ prm, int B, int chunks,
                                                              PprodIO io) {
  __shared__ __attribute__((aligned(16))) double smem[Q_TOTAL];
  const int b = blockIdx.x, chunk = blockIdx.y;
  if (b >= B) return;
  Solver<CapEv> S{};
  LDS double* sm = (LDS double*)smem;
  GLB double* gw = (GLB double*)(io.ws + ((long long)b * chunks + chunk) * kPprodWs);
  bind_solver(S, prm, sm, gw, b, kProdU, kProdGl, kProdHl, kProdTc, kProdDc);
  GLB double* oc = gw + kPprodOc;
  LDS double* dX = sm + Q_DX;
  // lane k's copy of xi_k[0:2] moved for one obstacle row: components 0 and 1 of its own row of
  // the prefix-sum scratch, which the tangent's sums (components 5..7) never use and which is
  // dead between those sums and the adjoint sweep, whose first pass rewrites each lane's own row
  LDS double* dXo = S.inc;
  LDS double* cr = sm + Q_CR;
  LDS double* dpl = sm + Q_DP;
  const int N = S.N, m = S.m, nb = S.nb, nw = S.nw, ng = S.ng, nwE = S.nwE, np = prm->np, npE = prm->npE;
  const int nxE = prm->nxE, nXE = nxE * (N + 1);
  const int w1p = prm->w1p, w2p = prm->w2p;
  const double sig = io.obj_factor;
  const int lane = S.lanef();
  const double* yb = io.lam_g ? io.lam_g + (long long)b * io.ld_lam_g : nullptr;
  const double* xb = io.x + (long long)b * io.ld_x;
  const double* db = io.dp ? io.dp + (long long)b * io.ld_dp : nullptr;

  // ---------------- scenario data (load_params' and load_controls' text)
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

  // ---------------- cost weights from p: unit-weight costs and gradients, lane k stage k's
  double c10 = 0.0, c01 = 0.0, g10[6], g01[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) g10[a] = g01[a] = 0.0;
  if (w1p >= 0 || w2p >= 0) {
    const double w1s = S.rvars[30], w2s = S.rvars[31];
    sync();
    if (w1p >= 0) {
      if (lane == 0) { S.rvars[30] = 1.0; S.rvars[31] = 0.0; }
      sync();
      c10 = k < N ? S.stage_cost(S.X + k * 8) : 0.0;
      S.derivs<false, true>(S.X, S.U, S.tc);
      if (k < N) {
#pragma unroll
        for (int a = 0; a < 6; ++a) g10[a] = S.gl[k * 8 + sv[a]];
      }
    }
    if (w2p >= 0) {
      if (lane == 0) { S.rvars[30] = 0.0; S.rvars[31] = 1.0; }
      sync();
      c01 = k < N ? S.stage_cost(S.X + k * 8) : 0.0;
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
  if (k < N) {
#pragma unroll
    for (int t = 0; t < 21; ++t) Hc[t] = sig * S.Hl[k * 21 + t];
  }
  if (k <= N && yb) {  // y-weighted obstacle curvature (obstacle_curvature's text), rows in order
    const LDS double* xk = S.X + k * 8;
    for (int o = 0; o < S.nobs; ++o) {
      const double C = yb[k * m + nb + o];
      const double ddx = xk[0] - S.obx[o], ddy = xk[1] - S.oby[o];
      const double idd = rsq(ddx * ddx + ddy * ddy);
      const double id3 = idd * idd * idd;
      const double h00 = C * (-ddy * ddy * id3), h01 = C * (ddx * ddy * id3), h11 = C * (-ddx * ddx * id3);
      q00 += h00; q01 += h01; q11 += h11;
      if (prm->oxp[o] >= 0 || prm->oyp[o] >= 0) {
        GLB double* q = oc + (k * NMPC_MAX_OBS + o) * 3;
        q[0] = h00; q[1] = h01; q[2] = h11;
      }
    }
  }
  if (k < N) {  // second derivatives of lam_{k+1}^T T f(x_k, u_k) (point_dyn2's text)
    const LDS double* tg = S.trig + k * 8;
    const double ct = tg[0], stt = tg[1], cp = tg[2], sp = tg[3], v = tg[4];
    const LDS double* ln = S.lam + (k + 1) * 8;
    const double l0 = ln[0], l1 = ln[1], l2 = ln[2];
    const double T = S.T;
    d33 = T * (-l0 * v * cp * ct - l1 * v * sp * ct - l2 * v * stt);
    d44 = T * (-l0 * v * cp * ct - l1 * v * sp * ct);
    d34 = T * (l0 * v * sp * stt - l1 * v * cp * stt);
    s03 = T * (-l0 * cp * stt - l1 * sp * stt + l2 * ct);
    s04 = T * (-l0 * sp * ct + l1 * cp * ct);
  }

  // ---------------- grad_p L (wavefront (b, 0); lane i forms internal entry i)
  if (io.gp && chunk == 0) {
    const double gxt = -(sig * wsum(k < N ? S.gl[k * 8] : 0.0));
    const double gyt = -(sig * wsum(k < N ? S.gl[k * 8 + 1] : 0.0));
    double v = 0.0;
    if (lane < 8) v = S.lam[lane];
    else if (lane == 8) v = gxt;
    else if (lane == 9) v = gyt;
    if (w1p >= 0) {
      const double s = sig * wsum(c10);
      if (lane == w1p) v += s;
    }
    if (w2p >= 0) {
      const double s = sig * wsum(c01);
      if (lane == w2p) v += s;
    }
    if (yb) {
      for (int o = 0; o < S.nobs; ++o) {
        if (prm->oxp[o] < 0 && prm->oyp[o] < 0) continue;
        double cx = 0.0, cy = 0.0;
        if (k <= N) {  // row g = r_sum - |(x, y) - (ox, oy)|: dg/dox = (x - ox) / d
          const double lg = yb[k * m + nb + o];
          const LDS double* xk = S.X + k * 8;
          const double ddx = xk[0] - S.obx[o], ddy = xk[1] - S.oby[o];
          const double idd = rsq(ddx * ddx + ddy * ddy);
          cx = lg * (ddx * idd);
          cy = lg * (ddy * idd);
        }
        cx = wsum(cx); cy = wsum(cy);
        if (lane == prm->oxp[o]) v += cx;
        if (lane == prm->oyp[o]) v += cy;
      }
    }
    const int e = lane < np ? ext_p(prm, lane) : -1;
    if (e >= 0) io.gp[(long long)b * npE + e] = v;
  }

  // which entries of a direction something reads (lane i: internal entry i)
  bool reads = lane < 10;
  if (lane == w1p || lane == w2p) reads = true;
  for (int o = 0; o < S.nobs; ++o)
    if (lane == prm->oxp[o] || lane == prm->oyp[o]) reads = true;
  const int pe = lane < np ? ext_p(prm, lane) : -1;
  reads = reads && pe >= 0;
  sync();  // lam is rewritten by every direction's sweep

  // ---------------- directions c, c + chunks, ...
  for (int d = chunk; d < io.nd; d += chunks) {
    // 6. the direction
    dpl[lane] = reads ? db[(long long)d * npE + pe] : 0.0;
    sync();
    // 7. state tangent
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
      for (int c = 0; c < 8; ++c) dX[k * 8 + c] = dx[c];
    }
    // 8. h_k, and the cross term of step 11
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
          for (int q = 0; q < 6; ++q) acc += Hc[hp(a, q)] * xs[q];
          hs[a] = acc;
        }
        if (w1p >= 0) {
          const double s = sig * dpl[w1p];
#pragma unroll
          for (int a = 0; a < 6; ++a) hs[a] += s * g10[a];
        }
        if (w2p >= 0) {
          const double s = sig * dpl[w2p];
#pragma unroll
          for (int a = 0; a < 6; ++a) hs[a] += s * g01[a];
        }
      }
      if (yb && S.nobs > 0) {
        hs[0] += q00 * dx[0] + q01 * dx[1];
        hs[1] += q01 * dx[0] + q11 * dx[1];
        for (int o = 0; o < S.nobs; ++o) {  // an obstacle's own move, against its own curvature
          const int ix = prm->oxp[o], iy = prm->oyp[o];
          if (ix < 0 && iy < 0) continue;
          const GLB double* q = oc + (k * NMPC_MAX_OBS + o) * 3;
          if (ix >= 0) { hs[0] -= q[0] * dpl[ix]; hs[1] -= q[1] * dpl[ix]; }
          if (iy >= 0) { hs[0] -= q[1] * dpl[iy]; hs[1] -= q[2] * dpl[iy]; }
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
    // 9. (dg/dp) dp and the tangent out
    if (io.jp && k <= N) {
      double* o = io.jp + ((long long)b * io.nd + d) * ng;
      for (int i = 0; i < m; ++i) {
        const int r = k * m + i;
        if (i < nb) {
          o[r] = S.row_jd(r, dX);
        } else {  // the row sees its obstacle's move as the opposite move of (x, y)
          const int ix = prm->oxp[i - nb], iy = prm->oyp[i - nb];
          dXo[k * 8] = ix >= 0 ? dx[0] - dpl[ix] : dx[0];
          dXo[k * 8 + 1] = iy >= 0 ? dx[1] - dpl[iy] : dx[1];
          o[r] = S.row_jd(r, dXo);
        }
      }
    }
    if (io.dXp) {
      double* o = io.dXp + ((long long)b * io.nd + d) * nXE;
      for (int i = lane; i < prm->nX; i += WAVE) {
        const int kk = i >> 3, c = i & 7;
        if (c < nxE) o[kk * nxE + c] = dX[i];
      }
    }
    if (!io.hp) {
      sync();
      continue;
    }
    // 10. mu_k = h_k + A_k^T mu_{k+1}
    S.adjoint(1.0, (const double*)nullptr);
    // 11. (d_p grad_w L dp)_{u_k}
    double* o = io.hp + ((long long)b * io.nd + d) * nwE;
    for (int i = lane; i < nw; i += WAVE) {
      const int e = ext_u(prm, i);
      if (e < 0) continue;
      const int kk = i / 6;
      const double g = S.grad_u(i);
      o[e] = i == 6 * kk ? g + cr[kk] : g;
    }
    sync();
  }
}

}  // namespace

int nmpc_pproducts_launch(const Params* dprm, int B, int chunks, const PprodIO& io, void* stream) {
  hipLaunchKernelGGL(nmpc_pproducts_kernel, dim3(B, chunks), dim3(WAVE), 0, (hipStream_t)stream, dprm, B, chunks, io);
  return (int)hipGetLastError();
}
