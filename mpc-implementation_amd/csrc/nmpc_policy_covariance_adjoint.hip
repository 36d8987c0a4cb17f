// nmpc_policy_covariance_adjoint.hip -- the reverse sweep of the policy covariance
// (nmpc_policy_covariance_adjoint_batch / nmpc_policy_covariance_adjoint_batch_dev,
// include/nmpc_amd.h): for each of B scenarios and each of nc cases, at the covariances Sigma_k the
// forward launch returned, the gradient of
//   L = sum_k <Sb_k, Sigma_k> + <ub, var_u> + <gb, var_g>
// with respect to S0, W, obs_var, K, ubar, Xbar and p.  With sym(S) = (S + S^T) / 2 and R_k the
// rows' terms (a box row adds gb[k,i] to Lam[bi,bi]; an obstacle row o adds gb[k,o] g g^T to
// Lam[0:2,0:2], gb[k,o] to obs_var_bar[o] and pos = H_o (2 gb[k,o] Sigma_k[0:2,0:2] g) to
// Xbar_bar[k,0:2], and -pos to its centre's entries of p_bar),
//   Lam_N = sym(Sb_N) + R_N
//   k = N-1 ... 0:  W_bar += Lam_{k+1}
//                   M = Lam_{k+1} Acl_k,   G = 2 M Sigma_k
//                   K_bar_k = B_k^T G + 2 diag(ub_k) K_k Sigma_k
//                   (Xbar_bar_k, ubar_bar_k) += <G, dA_k> + <G K_k^T, dB_k> pulled back through the eight
//                                               entries of A_k, B_k that depend on theta, psi and v
//                   Lam_k = Acl_k^T M + sym(Sb_k) + K_k^T diag(ub_k) K_k + R_k
//   S0_bar = Lam_0
// Lam_k is the gradient with respect to a covariance injected at stage k (a stage-varying W).
//
// Part of the evaluation kernel's translation unit (nmpc_policy_covariance.hip includes this file at
// its end): kCovStride, kCovMat and cov_acl are the forward kernel's, and A_k, B_k are Solver::stage_AB's
// entries in the forward kernel's own expressions, so Acl_k is the forward's bitwise.
//
// Execution model: the forward kernel's.  One wavefront per (scenario, case) on a grid of B x nc;
// lane = entry (i, j), i = lane % 8, j = lane / 8; matrices in LDS at a row stride of kCovStride
// doubles; every loop over a matrix dimension unrolled over 8 behind the wave-uniform guard l < nx.
// Symmetry: lane (i, j) forms the entry (max(i, j), min(i, j)) of Acl^T M and of every added term, so
// the two lanes of a mirrored pair perform the same operations on the same values and Lam is
// symmetric bitwise (sym(Sb): each lane loads Sb[i, j] and takes Sb[j, i] from its mirrored lane); only
// the lower triangle of each Sigma block is read.
// The serial chain is Lam alone: the sines, cosines and speed of every stage are formed once before
// the loop (lane = stage); stage k - 1's global loads (its K block, its Sigma block, its seeds) are
// issued at the top of stage k and consumed at its end, into the second buffers of Acl, K and Sigma.
// Row lane t < m holds row t of a stage.  The obstacle rows' sums over the lanes (Lam[0:2,0:2],
// Xbar_bar[k,0:2]) are the solver's wave sum, whose order depends on the lane numbers alone; p_bar and
// obs_var_bar accumulate over the stages, k = N ... 0, in the lane that holds the obstacle, and the
// obstacles that name one entry of p are added in ascending obstacle order.  W_bar accumulates
// Lam_N, Lam_{N-1}, ..., Lam_1 in that order.  No floating-point atomics, no workspace; plain C++
// stores only; no dynamically indexed private array.
// (included by nmpc_policy_covariance.hip)

namespace {

// LDS carve-up (doubles)
constexpr int CA_PP = 0;                          // p, internal layout (<= 64)
constexpr int CA_OB = CA_PP + 64;                 // obstacle x (16), y (16); at the end their p_bar terms
constexpr int CA_XY = CA_OB + 2 * NMPC_MAX_OBS;   // Xbar's position, 2 per stage
constexpr int CA_TR = CA_XY + 2 * kEvalStages;    // cos theta, sin theta, cos psi, sin psi, v: 5 per stage
constexpr int CA_LM = CA_TR + 5 * kEvalStages;    // Lam_{k+1}, then Lam_k
constexpr int CA_MM = CA_LM + kCovMat;            // M = Lam_{k+1} Acl_k
constexpr int CA_GG = CA_MM + kCovMat;            // G = 2 M Sigma_k
constexpr int CA_AC = CA_GG + kCovMat;            // Acl_k, Acl_{k-1} (two buffers)
constexpr int CA_KL = CA_AC + 2 * kCovMat;        // K_k, K_{k-1} (two buffers, rows r < 6)
constexpr int CA_SG = CA_KL + 2 * kCovMat;        // Sigma_k, Sigma_{k-1} (two buffers)
constexpr int CA_TOTAL = CA_SG + 2 * kCovMat;
// LDS for 16 wavefronts per CU within its 160 KB, as the forward kernel: the stage entries are kept
// as five factors per stage, not eight products, to stay under it with nine matrices.  (The registers
// hold 12: 132 VGPRs, 3 wavefronts per SIMD; a budget of 128 spills 20 bytes per lane to scratch.)
static_assert(CA_TOTAL * 8 <= 160 * 1024 / 16, "policy covariance adjoint kernel LDS");

// sym(Sb)'s entry from this lane's Sb[i, j] and the mirrored lane's Sb[j, i]: the sum is the same
// in both lanes of a pair (addition commutes bitwise), and a diagonal lane gets its own entry back
__device__ __forceinline__ double cov_sym(double v, int mirror) { return 0.5 * (v + __shfl(v, mirror, WAVE)); }

// one stage's global loads, held in registers from the top of the stage before to its end
struct CovAdjLoad {
  double kown, kacl;  // K_k: this lane's entry (r = i, j), and the entry its row of B_k K_k reads
  double sig;         // Sigma_k's lower-triangle entry (hi, lo)
  double sb;          // Sb_k[i, j]: the mirrored lane holds Sb_k[j, i]
  double gbox, gobs;  // gb of the box row on state i (lanes i == j), of this lane's obstacle row
  double ub[6];       // ub_k (wave-uniform addresses)
};

__global__ __launch_bounds__(WAVE) void nmpc_policy_covariance_adjoint_kernel(const Params* __restrict__ prm, int B,
                                                                              int nc, CovAdjIO io) {
  __shared__ __attribute__((aligned(16))) double smem[CA_TOTAL];
  const int b = blockIdx.x, cs = blockIdx.y;
  if (b >= B || cs >= nc) return;
  LDS double* sm = (LDS double*)smem;
  LDS double* pp = sm + CA_PP;
  LDS double* obx = sm + CA_OB;
  LDS double* oby = obx + NMPC_MAX_OBS;
  LDS double* xy = sm + CA_XY;
  LDS double* tr = sm + CA_TR;
  LDS double* lm = sm + CA_LM;
  LDS double* mm = sm + CA_MM;
  LDS double* gg = sm + CA_GG;
  const int N = prm->N, m = prm->m, nb = prm->nb, nobs = prm->nobs, nuE = prm->nuE, nxE = prm->nxE;
  const int nwE = prm->nwE, ng = prm->ng, npE = prm->npE, nn = nxE * nxE;
  const double T = prm->T;
  const int lane = threadIdx.x;
  const int i = lane & 7, j = lane >> 3;
  const bool act = i < nxE && j < nxE;       // an entry of the nx x nx matrices
  const bool kact = i < nuE && j < nxE;      // an entry (r = i, j) of the nu x nx gain
  const int hi = i > j ? i : j, lo = i > j ? j : i;  // the lower-triangle entry this lane forms
  const int kr = i < 3 ? 0 : i - 2;          // row of K that row i of B_k K_k reads (B_k: column 0, then T)
  const long long col = (long long)b * nc + cs;

  // ---------------- scenario data (as the forward kernel loads it)
  for (int q = lane; q < prm->np; q += WAVE) {
    const int e = ext_p(prm, q);
    pp[q] = e >= 0 ? io.p[(long long)b * io.ld_p + e] : 0.0;
  }
  for (int q = lane; q < 9 * kCovMat; q += WAVE) lm[q] = 0.0;  // Lam, M, G, Acl x 2, K x 2, Sigma x 2
  sync();
  if (lane < NMPC_MAX_OBS) {
    const bool on = lane < nobs;
    obx[lane] = on ? (prm->oxp[lane] >= 0 ? pp[prm->oxp[lane]] : prm->ox[lane]) : 0.0;
    oby[lane] = on ? (prm->oyp[lane] >= 0 ? pp[prm->oyp[lane]] : prm->oy[lane]) : 0.0;
  }
  // ---------------- lane k: Xbar_k's position, and the factors of stage k's A / B entries
  const double* Xb = io.Xbar + (long long)b * io.ld_Xbar;
  if (lane <= N) {
    xy[lane * 2] = Xb[lane * nxE];
    xy[lane * 2 + 1] = Xb[lane * nxE + 1];
  }
  if (lane < N) {
    const int k = lane;
    const double th = Xb[k * nxE + 3], ps = Xb[k * nxE + 4];
    LDS double* t = tr + k * 5;
    t[0] = cos(th); t[1] = sin(th); t[2] = cos(ps); t[3] = sin(ps);
    t[4] = io.ubar[(long long)b * io.ld_ubar + k * nuE];
  }

  // wave-uniform bases; the rows this lane serves
  const double* Kb = io.K ? io.K + (long long)b * io.ld_K : nullptr;
  const double* Sg = io.Sigma + (long long)b * io.ld_Sigma + (long long)cs * nn * (N + 1);
  const double* Sbs = io.Sigma_bar ? io.Sigma_bar + (long long)b * io.ld_Sigma_bar + (long long)cs * nn * (N + 1) : nullptr;
  const double* Ubs = (io.var_u_bar && Kb) ? io.var_u_bar + (long long)b * io.ld_var_u_bar + (long long)cs * nwE : nullptr;
  const double* Gbs = io.var_g_bar ? io.var_g_bar + (long long)b * io.ld_var_g_bar + (long long)cs * ng : nullptr;
  const int t_row = lane;                     // the row of a stage this lane holds
  const bool isobs = t_row >= nb && t_row < m;
  const int ob = isobs ? t_row - nb : 0;
  int brow = -1;                              // the box row on state i, for the diagonal lanes
#pragma unroll
  for (int t = 0; t < 5; ++t)
    if (t < nb && i == j && boxidx(t) == i) brow = t;
  const bool rows_on = Gbs && nobs > 0;       // wave-uniform: the obstacle rows are seeded
  double* Lo = io.Lambda ? io.Lambda + col * nn * (N + 1) : nullptr;
  double* Ko = io.K_bar ? io.K_bar + col * (long long)nuE * nxE * N : nullptr;
  double* Uo = io.ubar_bar ? io.ubar_bar + col * nwE : nullptr;
  double* Xo = io.Xbar_bar ? io.Xbar_bar + col * nxE * (N + 1) : nullptr;

  auto st_load = [&](int k) {  // wave-uniform k; k < 0: nothing
    CovAdjLoad q{};
    if (k < 0) return q;
    if (Kb && k < N) {
      const double* Kk = Kb + k * nuE * nxE;
      if (kact) q.kown = Kk[j * nuE + i];
      if (act) q.kacl = Kk[j * nuE + kr];
    }
    if (act) {
      q.sig = Sg[k * nn + lo * nxE + hi];
      if (Sbs) q.sb = Sbs[k * nn + j * nxE + i];
    }
    if (Gbs) {
      if (brow >= 0) q.gbox = Gbs[k * m + brow];
      if (isobs) q.gobs = Gbs[k * m + t_row];
    }
    if (Ubs && k < N) {
#pragma unroll
      for (int r = 0; r < 6; ++r)
        if (r < nuE) q.ub[r] = Ubs[k * nuE + r];
    }
    return q;
  };
  // stage k's Acl_k, K_k and Sigma_k into their LDS buffers, and this lane's obstacle row's
  // gradient g and 1 / d at Xbar_k: the row's Hessian in (x, y) is H = -(I - g g^T) / d (oracle
  // obstacle_derivs' entries -dy^2 / d^3, dx dy / d^3, -dx^2 / d^3)
  double gx = 0.0, gy = 0.0, idd = 0.0;
  auto stage_form = [&](int k, const CovAdjLoad& q) {
    if (k < 0) return;
    if (isobs) {
      const double ddx = xy[k * 2] - obx[ob], ddy = xy[k * 2 + 1] - oby[ob];
      const double d = sqrt(ddx * ddx + ddy * ddy);
      gx = -(ddx / d);
      gy = -(ddy / d);
      idd = 1.0 / d;
    }
    LDS double* sk = sm + CA_SG + (k & 1) * kCovMat;
    if (act) sk[i * kCovStride + j] = q.sig;
    if (k >= N) return;  // wave-uniform: stage N has rows only
    const LDS double* t = tr + k * 5;
    const double ct = t[0], stt = t[1], cp = t[2], sp = t[3], v = t[4];
    double a = i == j ? 1.0 : 0.0;
    if (i == 0 && j == 3) a = -T * v * cp * stt;  // E03
    if (i == 0 && j == 4) a = -T * v * sp * ct;   // E04
    if (i == 1 && j == 3) a = -T * v * sp * stt;  // E13
    if (i == 1 && j == 4) a = T * v * cp * ct;    // E14
    if (i == 2 && j == 3) a = T * v * ct;         // E23
    if (Kb) {
      double bik = T;
      if (i == 0) bik = T * cp * ct;  // b00
      if (i == 1) bik = T * sp * ct;  // b10
      if (i == 2) bik = T * stt;      // b20
      a = cov_acl(a, bik, q.kacl);
    }
    LDS double* ac = sm + CA_AC + (k & 1) * kCovMat;
    LDS double* kl = sm + CA_KL + (k & 1) * kCovMat;
    if (act) ac[i * kCovStride + j] = a;
    if (kact) kl[i * kCovStride + j] = q.kown;
  };
  // the rows' terms R_k at Sigma_k (sk): returns what this lane's entry of Lam_k gains; the
  // obstacle rows' pull-back to Xbar_k's position in (px, py)
  double pbx = 0.0, pby = 0.0, ovb = 0.0, px = 0.0, py = 0.0;
  auto rows = [&](const CovAdjLoad& q, const LDS double* sk) {
    double add = 0.0;
    px = 0.0;
    py = 0.0;
    if (!Gbs) return add;  // wave-uniform
    if (brow >= 0) add = q.gbox;
    if (rows_on) {
      const double s00 = sk[0], s10 = sk[kCovStride], s11 = sk[kCovStride + 1];
      const double gb = isobs ? q.gobs : 0.0;
      const double r00 = wsum(isobs ? gb * (gx * gx) : 0.0);
      const double r10 = wsum(isobs ? gb * (gx * gy) : 0.0);
      const double r11 = wsum(isobs ? gb * (gy * gy) : 0.0);
      const double ex = 2.0 * gb * (s00 * gx + s10 * gy), ey = 2.0 * gb * (s10 * gx + s11 * gy);
      const double cr = idd * (gx * ey - gy * ex);  // H (ex, ey) = (gy, -gx) cr
      const double pos0 = isobs ? gy * cr : 0.0;
      const double pos1 = isobs ? -(gx * cr) : 0.0;
      px = wsum(pos0);
      py = wsum(pos1);
      pbx = pbx - pos0;
      pby = pby - pos1;
      ovb = ovb + gb;
      if (hi == 0) add = r00;            // (0, 0) is no box state
      if (hi == 1 && lo == 0) add = r10;
      if (hi == 1 && lo == 1) add = r11;
    }
    return add;
  };

  sync();  // (tr, xy and the centres stand)
  // ---------------- stage N: Lam_N = sym(Sb_N) + R_N
  CovAdjLoad cur = st_load(N);
  stage_form(N, cur);
  sync();
  double lam = 0.0;
  {
    const double r = rows(cur, sm + CA_SG + (N & 1) * kCovMat);
    const double sy = cov_sym(cur.sb, j + 8 * i);
    lam = act ? sy + r : 0.0;
    if (Lo && act) Lo[N * nn + j * nxE + i] = lam;
    if (Xo && lane < nxE) Xo[N * nxE + lane] = lane == 0 ? px : (lane == 1 ? py : 0.0);
  }
  CovAdjLoad nxt = st_load(N - 1);
  stage_form(N - 1, nxt);
  if (act) lm[i * kCovStride + j] = lam;
  sync();

  double wacc = 0.0;
  for (int k = N - 1; k >= 0; --k) {
    cur = nxt;
    nxt = st_load(k - 1);
    const LDS double* ac = sm + CA_AC + (k & 1) * kCovMat;
    const LDS double* kl = sm + CA_KL + (k & 1) * kCovMat;
    const LDS double* sk = sm + CA_SG + (k & 1) * kCovMat;
    wacc = wacc + lam;
    // ---------------- M = Lam_{k+1} Acl_k; this lane's column of Sigma_k
    {
      double mv = 0.0;
#pragma unroll
      for (int l = 0; l < 8; ++l) {
        if (l < nxE) mv += lm[i * kCovStride + l] * ac[l * kCovStride + j];
      }
      mm[i * kCovStride + j] = mv;
    }
    double s[8];
#pragma unroll
    for (int l = 0; l < 8; ++l) s[l] = l < nxE ? sk[l * kCovStride + j] : 0.0;
    sync();  // (M stands)
    // ---------------- G = 2 M Sigma_k, and (K_k Sigma_k)[r = i, j]
    {
      double gv = 0.0;
#pragma unroll
      for (int l = 0; l < 8; ++l) {
        if (l < nxE) gv += mm[i * kCovStride + l] * s[l];
      }
      gg[i * kCovStride + j] = 2.0 * gv;
    }
    double pk = 0.0;
    if (Ubs && Ko) {  // wave-uniform
      const int r = i < 6 ? i : 5;  // (rows 6, 7 hold no gain: nu <= 6)
#pragma unroll
      for (int l = 0; l < 8; ++l) {
        if (l < nxE) pk += kl[r * kCovStride + l] * s[l];
      }
    }
    sync();  // (G stands)
    const LDS double* t = tr + k * 5;
    const double ct = t[0], stt = t[1], cp = t[2], sp = t[3], v = t[4];
    // ---------------- K_bar_k = B_k^T G + 2 diag(ub_k) K_k Sigma_k
    if (Ko) {
      double kb;
      if (i == 0) {
        kb = (T * cp * ct) * gg[j] + (T * sp * ct) * gg[kCovStride + j] + (T * stt) * gg[2 * kCovStride + j];
      } else {
        kb = T * gg[(i < 6 ? i + 2 : 7) * kCovStride + j];
      }
      if (Ubs) {
        double ubo = 0.0;  // ub_k[i]
#pragma unroll
        for (int q = 0; q < 6; ++q)
          if (i == q) ubo = cur.ub[q];
        kb = kb + 2.0 * ubo * pk;
      }
      if (kact) Ko[k * nuE * nxE + j * nuE + i] = kb;
    }
    // ---------------- the pull-back of <G, dA_k> + <G K_k^T, dB_k> to theta, psi and v
    const double r = rows(cur, sk);
    if (Xo || Uo) {
      double bb = 0.0;  // (G K_k^T)[i, 0]
      if (Kb) {
#pragma unroll
        for (int l = 0; l < 8; ++l) {
          if (l < nxE) bb += gg[i * kCovStride + l] * kl[l];
        }
      }
      const double bb0 = __shfl(bb, 0, WAVE), bb1 = __shfl(bb, 1, WAVE), bb2 = __shfl(bb, 2, WAVE);
      const double g03 = gg[3], g04 = gg[4], g13 = gg[kCovStride + 3], g14 = gg[kCovStride + 4];
      const double g23 = gg[2 * kCovStride + 3];
      const double thb = (-T * cp * stt) * bb0 + (-T * sp * stt) * bb1 + (T * ct) * bb2 + (-T * v * cp * ct) * g03 +
                         (T * v * sp * stt) * g04 + (-T * v * sp * ct) * g13 + (-T * v * cp * stt) * g14 +
                         (-T * v * stt) * g23;
      const double psb = (-T * sp * ct) * bb0 + (T * cp * ct) * bb1 + (T * v * sp * stt) * g03 +
                         (-T * v * cp * ct) * g04 + (-T * v * cp * stt) * g13 + (-T * v * sp * ct) * g14;
      const double vb = (-T * cp * stt) * g03 + (-T * sp * ct) * g04 + (-T * sp * stt) * g13 + (T * cp * ct) * g14 +
                        (T * ct) * g23;
      if (Xo && lane < nxE)
        Xo[k * nxE + lane] = lane == 0 ? px : (lane == 1 ? py : (lane == 3 ? thb : (lane == 4 ? psb : 0.0)));
      if (Uo && lane < nuE) Uo[k * nuE + lane] = lane == 0 ? vb : 0.0;
    }
    // ---------------- Lam_k: the lower-triangle entry (hi, lo) of Acl_k^T M + sym(Sb_k) + K_k^T diag(ub_k) K_k + R_k
    double ln = 0.0;
#pragma unroll
    for (int l = 0; l < 8; ++l) {
      if (l < nxE) ln += ac[l * kCovStride + hi] * mm[l * kCovStride + lo];
    }
    ln = ln + cov_sym(cur.sb, j + 8 * i);
    if (Ubs) {
      double kd = 0.0;
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        if (q < nuE) kd += kl[q * kCovStride + hi] * cur.ub[q] * kl[q * kCovStride + lo];
      }
      ln = ln + kd;
    }
    ln = ln + r;
    lam = act ? ln : 0.0;
    stage_form(k - 1, nxt);
    if (act) lm[i * kCovStride + j] = lam;
    if (Lo && act) Lo[k * nn + j * nxE + i] = lam;
    sync();
  }

  // ---------------- S0_bar = Lam_0, W_bar, and the obstacles' sums over the stages
  if (act) {
    if (io.S0_bar) io.S0_bar[col * nn + j * nxE + i] = lam;
    if (io.W_bar) io.W_bar[col * nn + j * nxE + i] = wacc;
  }
  if (io.obs_var_bar && isobs) io.obs_var_bar[col * nobs + ob] = ovb;
  if (io.p_bar) {  // exactly 0 outside the obstacle centres taken from p
    if (isobs) {
      obx[ob] = pbx;
      oby[ob] = pby;
    }
    sync();
    double mine = 0.0;
    for (int o = 0; o < nobs; ++o) {  // ascending obstacle order
      const int ex = prm->oxp[o] >= 0 ? ext_p(prm, prm->oxp[o]) : -1;
      const int ey = prm->oyp[o] >= 0 ? ext_p(prm, prm->oyp[o]) : -1;
      if (ex == lane) mine = mine + obx[o];
      if (ey == lane) mine = mine + oby[o];
    }
    if (lane < npE) io.p_bar[col * npE + lane] = mine;
  }
}

}  // namespace

int nmpc_policy_covariance_adjoint_launch(const Params* dprm, int B, int nc, const CovAdjIO& io, void* stream) {
  hipLaunchKernelGGL(nmpc_policy_covariance_adjoint_kernel, dim3(B, nc), dim3(WAVE), 0, (hipStream_t)stream, dprm, B,
                     nc, io);
  return (int)hipGetLastError();
}
