// nmpc_policy_covariance.hip -- closed-loop covariance of the plan's feedback policy and the
// standard deviations of its rows and controls (nmpc_policy_covariance_batch /
// nmpc_policy_covariance_batch_dev, include/nmpc_amd.h): for each of B scenarios and each of nc
// covariance cases the first-order propagation around the plan,
//   Sigma_0 = S0[c]
//   k = 0 ... N-1:  Acl_k      = A_k + B_k K_k                       (K null: A_k, open loop)
//                   var_u[k,r] = (K_k Sigma_k K_k^T)[r,r]            (K null: 0)
//                   var_g[k,i] = g_i^T Sigma_k g_i [+ obs_var[o]]    (g_i: the row's state gradient at Xbar_k)
//                   Sigma_{k+1} = Acl_k Sigma_k Acl_k^T + W[c]       (W null: no process noise)
//   var_g[N, .] at Sigma_N, Xbar_N;   sigma = sqrt(max(var, 0)), a NaN variance stays NaN.
// The analytic counterpart of nmpc_policy_rollout.hip: it reads the same p, ubar, Xbar and K.
//
// Part of the evaluation kernel's translation unit (nmpc_eval.hip includes this file last).  A_k and
// B_k are Solver::stage_AB's entries (oracle dyn_jac) at (Xbar_k, ubar_k); a box row's gradient is a
// unit vector, an obstacle row's -(x - ox, y - oy) / d.
//
// Execution model: one wavefront per (scenario, case) on a grid of B x nc; lane = entry (i, j) of
// the 8 x 8 matrix, i = lane % 8 the row and j = lane / 8 the column (the outputs' column-major
// order: with nx = 8 a block of Sigma_out is one coalesced run of 64 doubles).  Lanes with i or
// j >= nx carry zeros; every loop over a matrix dimension is unrolled over 8 behind the wave-uniform
// guard l < nx.  Sigma_k, Acl_k, K_k and the half product H = Acl_k Sigma_k sit in LDS at a row
// stride of kCovStride = 9 doubles: the lanes of a ds_read_b64 group read either one address per row
// i (8 rows, 18 dwords apart: distinct even banks) or a run of consecutive columns, and a
// ds_write_b64 group's 16 lanes (8 rows x 2 columns) fall on 16 distinct even banks of the 32; a
// stride of 8 would put the rows of one column on one bank (8-way).
// Symmetry: lane (i, j) forms the entry (max(i, j), min(i, j)) of H Acl^T + W, so the two lanes of a
// mirrored pair perform the same operations on the same values and Sigma is symmetric bitwise; only
// the lower triangles of S0 and W are read.
// The serial chain is Sigma alone.  What depends on Xbar, ubar and K only is formed off it: the
// transcendentals of every stage once before the loop (lane = stage), and Acl_{k+1}, K_{k+1} and the
// obstacle rows' gradients of stage k + 1 while stage k's products run -- their global loads are
// issued at the top of stage k and consumed at its end (as Solver::stage_ab in the solver's sweeps).
// Row variances: lane t < m holds row t of the stage, lane (r, j) with r < nu the term j of control
// r's quadratic form, reduced over j by three lane exchanges; sigma_g and sigma_u leave as runs of m
// and nu consecutive doubles from lanes 0 ... m - 1 and 0 ... nu - 1.  Plain C++ stores only.
// (included by nmpc_eval.hip)

namespace {

// LDS carve-up (doubles)
constexpr int kCovStride = 9;
constexpr int kCovMat = 8 * kCovStride;
constexpr int PC_PP = 0;                          // p, internal layout (<= 64)
constexpr int PC_OB = PC_PP + 64;                 // obstacle x (16), y (16)
constexpr int PC_XY = PC_OB + 2 * NMPC_MAX_OBS;   // Xbar's position, 2 per stage (the obstacle rows' gradients)
constexpr int PC_TR = PC_XY + 2 * kEvalStages;    // stage_AB's entries, 8 per stage: b00 b10 b20 E03 E04 E13 E14 E23
constexpr int PC_SG = PC_TR + 8 * kEvalStages;    // Sigma_k
constexpr int PC_HH = PC_SG + kCovMat;            // H = Acl_k Sigma_k
constexpr int PC_AC = PC_HH + kCovMat;            // Acl_k, Acl_{k+1} (two buffers)
constexpr int PC_KL = PC_AC + 2 * kCovMat;        // K_k, K_{k+1} (two buffers, rows r < 6)
constexpr int PC_TOTAL = PC_KL + 2 * kCovMat;
// 16 wavefronts per CU (4 per SIMD) within its 160 KB: 4,096 (scenario, case) pairs are then resident
// at once on the MI355X's 256 CUs instead of running a second, quarter-full round
static_assert(PC_TOTAL * 8 <= 160 * 1024 / 16, "policy covariance kernel LDS");

// sqrt(max(v, 0)) that keeps a NaN (fmax alone would drop it)
__device__ __forceinline__ double cov_sigma(double v) { return v > 0.0 ? sqrt(v) : (v != v ? v : 0.0); }

// an entry of Acl_k = A_k + B_k K_k: row i of B_k holds one entry bik (column 0 for the positions, T
// for an integrator state), and the product is rounded before the sum (no contraction).  Where the
// policy is deadbeat in a state, 1 + T K is ~1e-10 and that state's variance is set by the last bits of
// this sum: rounded so, the entry is the one fl(A + fl(B K)) that a matrix product in fp64 gives
__device__ __forceinline__ double cov_acl(double a, double bik, double kij) {
#pragma clang fp contract(off)
  const double bk = bik * kij;
  return a + bk;
}

__device__ __forceinline__ double cov_xchg(double v, int mask) { return __shfl_xor(v, mask, WAVE); }

__global__ __launch_bounds__(WAVE) void nmpc_policy_covariance_kernel(const Params* __restrict__ prm, int B, int nc,
                                                                      CovIO io) {
  __shared__ __attribute__((aligned(16))) double smem[PC_TOTAL];
  const int b = blockIdx.x, cs = blockIdx.y;
  if (b >= B || cs >= nc) return;
  LDS double* sm = (LDS double*)smem;
  LDS double* pp = sm + PC_PP;
  LDS double* obx = sm + PC_OB;
  LDS double* oby = obx + NMPC_MAX_OBS;
  LDS double* xy = sm + PC_XY;
  LDS double* tr = sm + PC_TR;
  LDS double* sg = sm + PC_SG;
  LDS double* hh = sm + PC_HH;
  const int N = prm->N, m = prm->m, nb = prm->nb, nobs = prm->nobs, nuE = prm->nuE, nxE = prm->nxE;
  const int nwE = prm->nwE, ng = prm->ng, nn = nxE * nxE;
  const double T = prm->T;
  const int lane = threadIdx.x;
  const int i = lane & 7, j = lane >> 3;
  const bool act = i < nxE && j < nxE;       // an entry of the nx x nx matrices
  const bool kact = i < nuE && j < nxE;      // an entry (r = i, j) of the nu x nx gain
  const int hi = i > j ? i : j, lo = i > j ? j : i;  // the lower-triangle entry this lane forms
  const int kr = i < 3 ? 0 : i - 2;          // row of K that row i of B_k K_k reads (B_k: column 0, then T)
  const long long col = (long long)b * nc + cs;

  // ---------------- scenario data (as the rollout kernel loads it)
  for (int q = lane; q < prm->np; q += WAVE) {
    const int e = ext_p(prm, q);
    pp[q] = e >= 0 ? io.p[(long long)b * io.ld_p + e] : 0.0;
  }
  for (int q = lane; q < 6 * kCovMat; q += WAVE) sg[q] = 0.0;  // Sigma, H, Acl x 2, K x 2
  sync();
  if (lane < NMPC_MAX_OBS) {
    const bool on = lane < nobs;
    obx[lane] = on ? (prm->oxp[lane] >= 0 ? pp[prm->oxp[lane]] : prm->ox[lane]) : 0.0;
    oby[lane] = on ? (prm->oyp[lane] >= 0 ? pp[prm->oyp[lane]] : prm->oy[lane]) : 0.0;
  }
  // ---------------- lane k: Xbar_k's position, and stage k's A / B entries (Solver::stage_AB at
  // Xbar_k, ubar_k)
  const double* Xb = io.Xbar + (long long)b * io.ld_Xbar;
  if (lane <= N) {
    xy[lane * 2] = Xb[lane * nxE];
    xy[lane * 2 + 1] = Xb[lane * nxE + 1];
  }
  if (lane < N) {
    const int k = lane;
    const double th = Xb[k * nxE + 3], ps = Xb[k * nxE + 4];
    const double v = io.ubar[(long long)b * io.ld_ubar + k * nuE];
    const double ct = cos(th), stt = sin(th), cp = cos(ps), sp = sin(ps);
    LDS double* t = tr + k * 8;
    t[0] = T * cp * ct; t[1] = T * sp * ct; t[2] = T * stt;  // b00, b10, b20
    t[3] = -T * v * cp * stt; t[4] = -T * v * sp * ct;   // E03, E04
    t[5] = -T * v * sp * stt; t[6] = T * v * cp * ct;    // E13, E14
    t[7] = T * v * ct;                                   // E23
  }

  // wave-uniform bases, this lane's entries of S0 and W (lower triangle) and its row's obs_var
  const double* Kb = io.K ? io.K + (long long)b * io.ld_K : nullptr;
  double sij = 0.0, wij = 0.0;
  if (act) {
    sij = io.S0[(long long)b * io.ld_S0 + (long long)cs * nn + lo * nxE + hi];
    if (io.W) wij = io.W[(long long)b * io.ld_W + (long long)cs * nn + lo * nxE + hi];
  }
  const int t_row = lane;                     // the row of a stage this lane holds
  const bool isobs = t_row >= nb && t_row < m;
  const int ob = isobs ? t_row - nb : 0;
  const int bi = t_row < nb ? boxidx(t_row) : 0;
  double ov = 0.0;
  if (isobs && io.obs_var) ov = io.obs_var[(long long)b * io.ld_obs_var + ob];
  double* So = io.Sigma ? io.Sigma + col * nn * (N + 1) : nullptr;
  double* Uo = io.sigma_u ? io.sigma_u + col * nwE : nullptr;
  double* Go = io.sigma_g ? io.sigma_g + col * ng : nullptr;

  // stage k's global loads of K: this lane's own entry (r = i, j) and the entry its row of B_k K_k reads
  struct KLoad { double own, acl; };
  auto k_load = [&](int k) {
    KLoad q{0.0, 0.0};
    if (Kb && k < N) {  // wave-uniform
      const double* Kk = Kb + (long long)k * nuE * nxE;
      if (kact) q.own = Kk[j * nuE + i];
      if (act) q.acl = Kk[j * nuE + kr];
    }
    return q;
  };
  // stage k's Acl_k and K_k into their LDS buffers, and this lane's obstacle row's gradient
  double gx = 0.0, gy = 0.0;
  auto stage_form = [&](int k, const KLoad& q) {
    if (isobs) {
      const double ddx = xy[k * 2] - obx[ob], ddy = xy[k * 2 + 1] - oby[ob];
      const double d = sqrt(ddx * ddx + ddy * ddy);
      gx = -(ddx / d);
      gy = -(ddy / d);
    }
    if (k >= N) return;  // wave-uniform: stage N has rows only
    const LDS double* t = tr + k * 8;
    double a = i == j ? 1.0 : 0.0;
    if (i == 0 && j == 3) a = t[3];
    if (i == 0 && j == 4) a = t[4];
    if (i == 1 && j == 3) a = t[5];
    if (i == 1 && j == 4) a = t[6];
    if (i == 2 && j == 3) a = t[7];
    if (Kb) a = cov_acl(a, i < 3 ? t[i] : T, q.acl);
    LDS double* ac = sm + PC_AC + (k & 1) * kCovMat;
    LDS double* kl = sm + PC_KL + (k & 1) * kCovMat;
    if (act) ac[i * kCovStride + j] = a;
    if (kact) kl[i * kCovStride + j] = q.own;
  };

  sync();  // (tr stands)
  stage_form(0, k_load(0));
  if (act) sg[i * kCovStride + j] = sij;
  sync();

  for (int k = 0; k <= N; ++k) {
    const KLoad kn = k_load(k + 1);
    const LDS double* ac = sm + PC_AC + (k & 1) * kCovMat;
    const LDS double* kl = sm + PC_KL + (k & 1) * kCovMat;
    // ---------------- this lane's column of Sigma_k; H = Acl_k Sigma_k and control r = i's term j
    double s[8];
#pragma unroll
    for (int l = 0; l < 8; ++l) s[l] = l < nxE ? sg[l * kCovStride + j] : 0.0;
    if (k < N) {
      double h = 0.0;
#pragma unroll
      for (int l = 0; l < 8; ++l) {
        if (l < nxE) h += ac[i * kCovStride + l] * s[l];
      }
      hh[i * kCovStride + j] = h;
      if (Uo) {
        double q = 0.0;
        if (Kb) {
          const int r = i < 6 ? i : 5;  // (rows 6, 7 of the buffer do not exist: nu <= 6)
          double pk = 0.0;
#pragma unroll
          for (int l = 0; l < 8; ++l) {
            if (l < nxE) pk += kl[r * kCovStride + l] * s[l];
          }
          q = kact ? pk * kl[r * kCovStride + j] : 0.0;
          q += cov_xchg(q, 8);
          q += cov_xchg(q, 16);
          q += cov_xchg(q, 32);
        }
        if (lane < nuE) Uo[k * nuE + lane] = cov_sigma(q);
      }
    }
    // ---------------- the stage's rows and Sigma_k out
    if (Go) {
      const double s00 = sg[0], s10 = sg[kCovStride], s11 = sg[kCovStride + 1];
      const double sbb = sg[bi * kCovStride + bi];
      const double vo = gx * (s00 * gx + s10 * gy) + gy * (s10 * gx + s11 * gy) + ov;
      if (t_row < m) Go[k * m + t_row] = cov_sigma(isobs ? vo : sbb);
    }
    if (So && act) So[(long long)k * nn + j * nxE + i] = sij;
    if (k == N) break;
    sync();  // (H stands)
    // ---------------- Sigma_{k+1}: the lower-triangle entry (hi, lo) of H Acl_k^T + W
    double sn = 0.0;
#pragma unroll
    for (int l = 0; l < 8; ++l) {
      if (l < nxE) sn += hh[hi * kCovStride + l] * ac[lo * kCovStride + l];
    }
    sn = sn + wij;
    sij = act ? sn : 0.0;
    stage_form(k + 1, kn);
    if (act) sg[i * kCovStride + j] = sij;
    sync();
  }
}

}  // namespace

int nmpc_policy_covariance_launch(const Params* dprm, int B, int nc, const CovIO& io, void* stream) {
  hipLaunchKernelGGL(nmpc_policy_covariance_kernel, dim3(B, nc), dim3(WAVE), 0, (hipStream_t)stream, dprm, B, nc, io);
  return (int)hipGetLastError();
}

// the reverse sweep of that covariance, one wavefront per (scenario, case) again: a twelfth kernel
// of this unit
#include "nmpc_policy_covariance_adjoint.hip"
