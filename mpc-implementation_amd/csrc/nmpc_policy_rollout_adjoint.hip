// nmpc_policy_rollout_adjoint.hip -- the reverse sweep of the policy rollouts
// (nmpc_policy_rollout_adjoint_batch / nmpc_policy_rollout_adjoint_batch_dev, include/nmpc_amd.h):
// for each of B scenarios with M samples, at the trajectories X the forward launch returned, the
// gradient of
//   L_b = sum_s ( Jb_s J_s + <Xb_s, X_s> + <Ub_s, U_s> )
// with respect to ubar, K, Xbar and p (summed over the scenario's samples) and to e0 and w (per
// sample).  Per sample, with x_k = X[s, k], backwards over the stages,
//   lam_N = Xb_N
//   k = N-1 ... 0:  u_raw, u_k as the forward kernel forms them; mask_r = (u_k[r] == u_raw[r])
//                   mu    = mask . (B_k^T lam_{k+1} + Ub_k)             A_k, B_k at (x_k, u_k)
//                   wbar_k = lam_{k+1}
//                   lam_k = Jb grad l_k(x_k) + Xb_k + A_k^T lam_{k+1} + K_k^T mu
//                   ubar_bar_k += mu,  K_bar_k += mu (x_k - Xbar_k)^T,  Xbar_bar_k -= K_k^T mu
//                   p_bar[target x, y] -= Jb (grad l_k)[0, 1]
//                   p_bar[w1 index] += Jb dd_k,  p_bar[w2 index] += Jb (Q_k - 1)
//   e0_bar = lam_0,  p_bar[x0 block] += lam_0
//
// Part of the evaluation kernel's translation unit (nmpc_eval.hip includes this file after
// nmpc_policy_rollout.hip, whose slot layout, LDS carve-up and clamp text it uses).  The stage
// cost's gradient is the gradient part of Solver::derivs (HESS = false, no cache) restated on a
// pointer to one state, as nmpc_point.hip restates the solver's steps; A_k and B_k are stage_AB's
// entries.
//
// Execution model: lane = sample, one wavefront per (scenario, block of 64 samples), the
// scenario's p, weights and Xbar in LDS, the lane's current state in its own LDS slot
// (kRollStride apart), K_k, ubar_k and the bounds read at wave-uniform addresses.  Lanes past M
// recompute sample M - 1, store nothing and enter every sum as an exact 0.  The sums over the 64
// lanes are the solver's wave sum (wsum: DPP within rows of 16, permlane swaps across them): the
// order of its additions depends on the lane numbers alone, never on the data.  A block's sums go
// straight to the outputs when M <= 64; with more blocks each writes its partial sums to the
// handle's workspace and nmpc_policy_rollout_adjoint_sum_kernel adds them in ascending block
// order.  No floating-point atomics; plain C++ stores only; no dynamically indexed private array.
// A NaN among a sample's states, seeds, controls or the bounds it meets makes that sample's e0_bar
// and w_bar NaN and, as a sum with a NaN term is, every entry of its scenario's reduced outputs
// that the rollout reads; other scenarios are untouched.
// (included by nmpc_eval.hip)

namespace {

// The gradient of the stage cost l(x; p) at the state x points to: Solver::derivs' gradient
// part, the same operations in the same order.  Returns the target distance dd and Q - 1 (the
// terms the cost weights multiply) for the weights' entries of p_bar.
__device__ __forceinline__ void roll_adj_cost_grad(const Solver<CapEv>& S, const LDS double* xk, double (&g8)[8],
                                                   double& dd_out, double& qm1_out) {
  const double hv = S.P->hv, hh = S.P->hh;
  const double x = xk[0], yy = xk[1], z = xk[2], x5 = xk[5], x6 = xk[6], x7 = xk[7];
  const double xt = S.pp[8], yt = S.pp[9];
  double t6p, t6m, t5p, t5m;
  Solver<CapEv>::tan_pm(x6, hv, S.P->thv, t6p, t6m);
  Solver<CapEv>::tan_pm(x5, hh, S.P->thh, t5p, t5m);
  const double al6 = (t6p - t6m) / 2, be6 = (t6p + t6m) / 2;
  const double al5 = (t5p - t5m) / 2, be5 = (t5p + t5m) / 2;
  const double al6d = (t6p * t6p - t6m * t6m) / 2, be6d = (2 + t6p * t6p + t6m * t6m) / 2;
  const double al5d = (t5p * t5p - t5m * t5m) / 2, be5d = (2 + t5p * t5p + t5m * t5m) / 2;
  const double ex = xt - x - z * be6;
  const double ey = yt - yy - z * be5;
  const double gex[6] = {-1.0, 0.0, -be6, 0.0, -z * be6d, 0.0};
  const double gey[6] = {0.0, -1.0, -be5, -z * be5d, 0.0, 0.0};
  const double a = z * al6, bb = z * al5;
  const double ga[6] = {0.0, 0.0, al6, 0.0, z * al6d, 0.0};
  const double gb[6] = {0.0, 0.0, al5, z * al5d, 0.0, 0.0};
  const double c = cos(x7), sn = sin(x7);
  const double r1 = c * ex + sn * ey;
  const double r2 = sn * ex - c * ey;
  const double ia = qd(1.0, a), ib = qd(1.0, bb);
  const double e1 = r1 * ia, e2 = r2 * ib;
  const double ddx = x - xt, ddy = yy - yt;
  const double dd = sqrt(ddx * ddx + ddy * ddy);
  const double idd = qd(1.0, dd);
  const double w1 = S.rvars[30], w2 = S.rvars[31];
  double g6[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    const double gr1 = c * gex[q] + sn * gey[q] - (q == 5 ? r2 : 0.0);
    const double gr2 = sn * gex[q] - c * gey[q] + (q == 5 ? r1 : 0.0);
    const double ge1 = (gr1 - e1 * ga[q]) * ia;
    const double ge2 = (gr2 - e2 * gb[q]) * ib;
    g6[q] = w2 * (2 * (e1 * ge1 + e2 * ge2));
  }
  g6[0] += w1 * (ddx * idd);
  g6[1] += w1 * (ddy * idd);
  g8[0] = g6[0]; g8[1] = g6[1]; g8[2] = g6[2]; g8[3] = 0.0; g8[4] = 0.0;
  g8[5] = g6[3]; g8[6] = g6[4]; g8[7] = g6[5];
  dd_out = dd;
  qm1_out = (e1 * e1 + e2 * e2) - 1;
}

// where a block's sums go: the caller's outputs (one block) or the block's slice of the workspace,
// laid out [ubar_bar (nw) | K_bar (nu nx N) | Xbar_bar (nx (N+1)) | p_bar (np)]
struct RollAdjDst { double *ubar, *K, *Xbar, *p; };

__global__ __launch_bounds__(WAVE) void nmpc_policy_rollout_adjoint_kernel(const Params* __restrict__ prm, int B,
                                                                           int M, RollAdjIO io) {
  __shared__ __attribute__((aligned(16))) double smem[PR_TOTAL];
  const int b = blockIdx.x;
  if (b >= B) return;
  Solver<CapEv> S{};
  LDS double* sm = (LDS double*)smem;
  S.P = (const CST Params*)prm; S.sm = sm; S.lane_ = threadIdx.x; S.b = b;
  S.N = prm->N; S.m = prm->m; S.nobs = prm->nobs; S.nw = prm->nw; S.ng = prm->ng; S.T = prm->T;
  S.nb = prm->nb; S.nuE = prm->nuE; S.nwE = prm->nwE;
  S.pp = sm + PR_PP; S.obx = sm + PR_OB; S.oby = S.obx + NMPC_MAX_OBS; S.rvars = sm + PR_RV;
  LDS double* xbar = sm + PR_XB;
  const int N = S.N, nuE = S.nuE, nwE = S.nwE, nxE = prm->nxE, nXE = nxE * (N + 1), npE = prm->npE;
  const int nKE = nuE * nxE * N;
  const double T = S.T;
  const int lane = S.lanef();
  const int nblk = gridDim.y, blk = blockIdx.y;
  const long long s = (long long)blk * WAVE + lane;
  const bool live = s < M;
  const long long sc = live ? s : M - 1;        // lanes past M recompute the last sample
  const long long col = (long long)b * M + sc;  // the sample's column of every per-sample output

  // ---------------- scenario data (as the forward kernel loads it, without the obstacle centres:
  // no row is evaluated here), and Xbar
  load_p(S, prm, lane, io.p + (long long)b * io.ld_p);
  sync();
  load_weights(S, prm, lane);
  {
    const double* Xb = io.Xbar + (long long)b * io.ld_Xbar;
    for (int i = lane; i < nXE; i += WAVE) {
      const int k = i / nxE, c = i - k * nxE;
      xbar[k * 8 + c] = Xb[i];
    }
  }
  sync();

  // wave-uniform bases
  const double* ub = io.ubar + (long long)b * io.ld_ubar;
  const double* Kb = io.K ? io.K + (long long)b * io.ld_K : nullptr;
  const double* lxb = io.lbx ? io.lbx + (long long)b * io.ld_lbx : nullptr;
  const double* uxb = io.ubx ? io.ubx + (long long)b * io.ld_ubx : nullptr;
  RollAdjDst dst;
  if (nblk == 1) {
    dst.ubar = io.ubar_bar ? io.ubar_bar + (long long)b * nwE : nullptr;
    dst.K = io.K_bar ? io.K_bar + (long long)b * nKE : nullptr;
    dst.Xbar = io.Xbar_bar ? io.Xbar_bar + (long long)b * nXE : nullptr;
    dst.p = io.p_bar ? io.p_bar + (long long)b * npE : nullptr;
  } else {
    double* part = io.ws + ((long long)b * nblk + blk) * (long long)(nwE + nKE + nXE + npE);
    dst.ubar = io.ubar_bar ? part : nullptr;
    dst.K = io.K_bar ? part + nwE : nullptr;
    dst.Xbar = io.Xbar_bar ? part + nwE + nKE : nullptr;
    dst.p = io.p_bar ? part + nwE + nKE + nXE : nullptr;
  }
  // per-lane bases
  const double* Xs = io.X + (long long)b * io.ld_X + sc * nXE;
  const double* Xbs = io.Xb ? io.Xb + (long long)b * io.ld_Xb + sc * nXE : nullptr;
  const double* Ubs = io.Ub ? io.Ub + (long long)b * io.ld_Ub + sc * nwE : nullptr;
  const double Jb = io.Jb ? io.Jb[(long long)b * io.ld_Jb + sc] : 0.0;
  double* e0o = io.e0_bar ? io.e0_bar + col * nxE : nullptr;
  double* wo = io.w_bar ? io.w_bar + col * (long long)N * nxE : nullptr;

  bool bad = Jb != Jb;
  int nsat = 0;
  // ---------------- lam_N = Xb_N (an absent gimbal state's costate stays 0)
  double lam[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    lam[c] = 0.0;
    if (c < nxE) {
      const double xn = Xs[N * nxE + c];
      bad |= xn != xn;
      if (Xbs) lam[c] = Xbs[N * nxE + c];
    }
    bad |= lam[c] != lam[c];
  }
  if (dst.Xbar && lane < nxE) dst.Xbar[N * nxE + lane] = 0.0;
  // what the lane adds to p_bar: the target's x and y, the two cost weights
  double ptx = 0.0, pty = 0.0, pw1 = 0.0, pw2 = 0.0;
  LDS double* xl = sm + PR_XL + lane * kRollStride;

  for (int k = N - 1; k >= 0; --k) {
    // ---------------- x_k to the lane's slot
    double x[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      x[c] = S.pp[c];
      if (c < nxE) x[c] = Xs[k * nxE + c];
      bad |= x[c] != x[c];
      xl[c] = x[c];
    }
    // ---------------- the clamped policy's control and the clamp's mask (the forward kernel's text)
    double u[6];
    bool mask[6];
    const double* Kk = Kb ? Kb + (long long)k * nuE * nxE : nullptr;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      u[r] = 0.0;
      mask[r] = false;
      if (r < nuE) {
        double ur = ub[k * nuE + r];
        if (Kk) {
          double acc = 0.0;
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            if (c < nxE) acc += Kk[c * nuE + r] * (x[c] - xbar[k * 8 + c]);
          }
          ur = ur + acc;
        }
        double uc = ur;
        if (lxb) {
          const double lo = lxb[k * nuE + r];
          uc = uc < lo ? lo : uc;
          bad |= lo != lo;
        }
        if (uxb) {
          const double hi = uxb[k * nuE + r];
          uc = uc > hi ? hi : uc;
          bad |= hi != hi;
        }
        bad |= ur != ur;
        nsat += (uc != ur && ur == ur) ? 1 : 0;
        mask[r] = uc == ur;
        u[r] = uc;
      }
    }
    // ---------------- A_k = I + E_k and B_k at (x_k, u_k): stage_AB's entries
    const double ct = cos(x[3]), stt = sin(x[3]), cp = cos(x[4]), sp = sin(x[4]);
    const double v = u[0];
    const double E03 = -T * v * cp * stt, E04 = -T * v * sp * ct;
    const double E13 = -T * v * sp * stt, E14 = T * v * cp * ct;
    const double E23 = T * v * ct;
    const double b00 = T * cp * ct, b10 = T * sp * ct, b20 = T * stt;
    // ---------------- mu = mask . (B_k^T lam_{k+1} + Ub_k), wbar_k = lam_{k+1}
    double mu[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      mu[r] = 0.0;
      if (r < nuE) {
        double t = r == 0 ? b00 * lam[0] + b10 * lam[1] + b20 * lam[2] : T * lam[2 + r];
        if (Ubs) {
          const double ubr = Ubs[k * nuE + r];
          bad |= ubr != ubr;
          t = t + ubr;
        }
        mu[r] = mask[r] ? t : 0.0;
      }
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (wo && live && c < nxE) wo[k * nxE + c] = lam[c];
    }
    // ---------------- K_k^T mu and the sums over the block's samples
    double ktm[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      ktm[c] = 0.0;
      if (Kk && c < nxE) {
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          if (r < nuE) ktm[c] += Kk[c * nuE + r] * mu[r];
        }
      }
    }
    if (dst.ubar) {
      double mine = 0.0;
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        if (r < nuE) {
          const double t = wsum(live ? mu[r] : 0.0);
          if (lane == r) mine = t;
        }
      }
      if (lane < nuE) dst.ubar[k * nuE + lane] = mine;
    }
    if (dst.K) {
      double mine = 0.0;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        if (c < nxE) {
          const double dxc = x[c] - xbar[k * 8 + c];
#pragma unroll
          for (int r = 0; r < 6; ++r) {
            if (r < nuE) {
              const double t = wsum(live ? mu[r] * dxc : 0.0);
              if (lane == c * nuE + r) mine = t;
            }
          }
        }
      }
      if (lane < nuE * nxE) dst.K[(long long)k * nuE * nxE + lane] = mine;
    }
    if (dst.Xbar) {
      double mine = 0.0;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        if (c < nxE) {
          const double t = wsum(live ? -ktm[c] : 0.0);
          if (lane == c) mine = t;
        }
      }
      if (lane < nxE) dst.Xbar[k * nxE + lane] = mine;
    }
    // ---------------- lam_k = Jb grad l_k + Xb_k + A_k^T lam_{k+1} + K_k^T mu
    double g8[8], dd = 0.0, qm1 = 0.0;
#pragma unroll
    for (int c = 0; c < 8; ++c) g8[c] = 0.0;
    if (io.Jb) {  // wave-uniform
      roll_adj_cost_grad(S, xl, g8, dd, qm1);
#pragma unroll
      for (int c = 0; c < 8; ++c) g8[c] = Jb * g8[c];
      ptx -= g8[0];
      pty -= g8[1];
      pw1 += Jb * dd;
      pw2 += Jb * qm1;
    }
    const double a3 = E03 * lam[0] + E13 * lam[1] + E23 * lam[2];
    const double a4 = E04 * lam[0] + E14 * lam[1];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      double t = lam[c];
      if (c == 3) t = t + a3;
      if (c == 4) t = t + a4;
      t = t + ktm[c];
      if (c < nxE) {
        t = t + g8[c];
        if (Xbs) {
          const double xbc = Xbs[k * nxE + c];
          bad |= xbc != xbc;
          t = t + xbc;
        }
        lam[c] = t;
      } else {
        lam[c] = 0.0;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) bad |= lam[c] != lam[c];

  // ---------------- per-sample outputs; a NaN met on the way poisons them
  const bool anybad = wany(bad && live);  // wave-uniform
  if (live) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (e0o && c < nxE) e0o[c] = bad ? NAN : lam[c];
    }
    if (io.nsat) io.nsat[col] = nsat;
    if (bad && wo)
      for (int i = 0; i < N * nxE; ++i) wo[i] = NAN;
  }
  // ---------------- p_bar: the x0 block, the target, the weights; exactly 0 elsewhere
  if (dst.p) {
    double mine = 0.0;
    bool read = false;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (c < nxE) {
        const double t = wsum(live ? lam[c] : 0.0);
        if (lane == c) { mine = t; read = true; }
      }
    }
    const int tx = ext_p(prm, 8), ty = ext_p(prm, 9);
    const int e1 = prm->w1p >= 0 ? ext_p(prm, prm->w1p) : -1, e2 = prm->w2p >= 0 ? ext_p(prm, prm->w2p) : -1;
    const double stx = wsum(live ? ptx : 0.0), sty = wsum(live ? pty : 0.0);
    if (lane == tx) { mine = stx; read = true; }
    if (lane == ty) { mine = sty; read = true; }
    if (e1 >= 0) {  // wave-uniform
      const double t = wsum(live ? pw1 : 0.0);
      if (lane == e1) { mine = t; read = true; }
    }
    if (e2 >= 0) {
      const double t = wsum(live ? pw2 : 0.0);
      if (lane == e2) { mine = t; read = true; }
    }
    if (lane < npE) dst.p[lane] = (read && anybad) ? NAN : mine;
  }
  if (anybad) {  // rare: as a sum with a NaN term, every reduced entry the rollout reads
    if (dst.ubar)
      for (int i = lane; i < nwE; i += WAVE) dst.ubar[i] = NAN;
    if (dst.K)
      for (int i = lane; i < nKE; i += WAVE) dst.K[i] = NAN;
    if (dst.Xbar)
      for (int i = lane; i < N * nxE; i += WAVE) dst.Xbar[i] = NAN;
  }
}

// M > 64: a scenario's per-block partial sums added in ascending block order, one thread per entry
__global__ __launch_bounds__(256) void nmpc_policy_rollout_adjoint_sum_kernel(const Params* __restrict__ prm, int B,
                                                                              int nblk, RollAdjIO io) {
  const int N = prm->N, nwE = prm->nwE, nxE = prm->nxE, nXE = nxE * (N + 1), npE = prm->npE;
  const int nKE = prm->nuE * nxE * N, nred = nwE + nKE + nXE + npE;
  const int b = blockIdx.x, i = blockIdx.y * 256 + threadIdx.x;
  if (b >= B || i >= nred) return;
  double* out;
  if (i < nwE) out = io.ubar_bar ? io.ubar_bar + (long long)b * nwE + i : nullptr;
  else if (i < nwE + nKE) out = io.K_bar ? io.K_bar + (long long)b * nKE + (i - nwE) : nullptr;
  else if (i < nwE + nKE + nXE) out = io.Xbar_bar ? io.Xbar_bar + (long long)b * nXE + (i - nwE - nKE) : nullptr;
  else out = io.p_bar ? io.p_bar + (long long)b * npE + (i - nwE - nKE - nXE) : nullptr;
  if (!out) return;
  const double* part = io.ws + (long long)b * nblk * nred + i;
  double acc = part[0];
  for (int j = 1; j < nblk; ++j) acc = acc + part[(long long)j * nred];
  *out = acc;
}

}  // namespace

int nmpc_policy_rollout_adjoint_launch(const Params* dprm, int B, int M, const RollAdjIO& io, int nred,
                                       void* stream) {
  const int nblk = (M + WAVE - 1) / WAVE;
  hipLaunchKernelGGL(nmpc_policy_rollout_adjoint_kernel, dim3(B, nblk), dim3(WAVE), 0, (hipStream_t)stream, dprm, B, M,
                     io);
  if (nblk > 1 && (io.ubar_bar || io.K_bar || io.Xbar_bar || io.p_bar))
    hipLaunchKernelGGL(nmpc_policy_rollout_adjoint_sum_kernel, dim3(B, (nred + 255) / 256), dim3(256), 0,
                       (hipStream_t)stream, dprm, B, nblk, io);
  return (int)hipGetLastError();
}
