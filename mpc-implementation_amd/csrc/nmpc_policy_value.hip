// nmpc_policy_value.hip -- the cost-to-go expansion of the plan's feedback policy
// (nmpc_policy_value_batch / nmpc_policy_value_batch_dev, include/nmpc_amd.h): for each of B
// scenarios the local quadratic model of the closed loop's cost from every stage on, and from it the
// expected cost and its variance under nc covariance cases,
//   lam_N = 0, P_N = 0
//   k = N-1 ... 0:  Acl_k = A_k + B_k K_k                          (K null: A_k, open loop)
//                   M_k   = H_k + Fxx + Fxu K_k + K_k^T Fxu^T      (H_k = grad^2 l_k; Fxx, Fxu the second
//                                                                  derivatives of lam_{k+1}^T T f)
//                   lam_k = g_k + Acl_k^T lam_{k+1}                (g_k = grad l_k)
//                   P_k   = M_k + Acl_k^T P_{k+1} Acl_k
//   J = sum_k l_k(Xbar_k);  dJ[c] = 1/2 <P_0, S0[c]> + 1/2 <P_N + ... + P_1, W[c]>
//   varJ[c] = lam_0^T S0[c] lam_0 + sum_{k >= 1} lam_k^T W[c] lam_k
// The second-order counterpart of nmpc_policy_covariance.hip: it reads the same p, ubar, Xbar and K.
//
// Part of the evaluation kernel's translation unit (nmpc_eval.hip includes this file after the
// rollout kernels), so the model is the text the solver compiles: Solver::stage_cost (l_k),
// Solver::derivs<true> (g_k, H_k and the cached cos / sin of theta, psi), Solver::stage_AB (A_k, B_k)
// and point_dyn2 (Fxx, Fxu).  Solver::derivs writes g_k and H_k through global pointers, so this
// kernel takes one products-kernel slice (kProdWs doubles) of the handle's workspace per scenario.
//
// Execution model: one wavefront per SCENARIO.  P_k does not depend on the case, so the cases are a
// loop of wave sums at the end, not a grid dimension.
//   1. scenario data, Xbar to the trajectory buffer, ubar to the workspace; lane k: l_k, g_k, H_k and
//      stage_AB's entries of stage k (nothing is rolled out: the expansion is at the points given);
//   2. lam: a serial sweep, lane i < 8 forming row i of g_k + Acl_k^T lam_{k+1};
//   3. lane k: point_dyn2's five terms of stage k with the solver's multiplier buffer holding
//      lam_{k+1}, as rounded products T e; lane (i, j): sum_{k >= 1} lam_k[i] lam_k[j];
//   4. P: lane = entry (i, j) of the 8 x 8 matrix, i = lane % 8 the row and j = lane / 8 the column,
//      as the covariance kernel.  P_{k+1}, Acl_k, K_k and the half product G = P_{k+1} Acl_k sit in
//      LDS at a row stride of kValStride = 9 doubles (that kernel's bank argument).  Lane (i, j) forms
//      the entry (max(i, j), min(i, j)) of M_k + Acl_k^T G, so the two lanes of a mirrored pair perform
//      the same operations on the same values and P_k is symmetric bitwise.
//      The serial chain is P alone: K_{k-1}, H_{k-1}'s entry and Acl_{k-1} are loaded and formed while
//      stage k's products run, and M_k's entry is formed before the barrier its half product waits at;
//   5. per case: the lower triangles of S0 and W against P_0, sum P_k, lam_0 lam_0^T and
//      sum lam_k lam_k^T, off-diagonal entries counted twice, through the solver's wsum.
// Rounding.  Acl_k's entries are rounded as the covariance kernel's: fl(A + fl(B K)), contraction
// off.  M_k's entry is fl(H + Fxx) with the two cross products then added by fused multiply-adds
// (fma(Fxu[hi], K[0, lo], .), then fma(K[0, hi], Fxu[lo], .)); Fxx and Fxu are rounded products T e.
// The dot products of lam_k, G and P_k are chains of fused multiply-adds in ascending l, P_k's
// starting from M_k's entry.
// A NaN in K or Xbar reaches lam_0 and P_0 through Acl_k (every sum is dense: 0 * NaN), and J is set
// to NaN where lam_0 holds one.  Plain C++ stores only, no atomics: two calls agree bitwise.
// (included by nmpc_eval.hip)

namespace {

static_assert(fits_every_class(kProdWs),
              "a solver class's workspace is smaller than one wavefront's of the policy value kernel");

// LDS carve-up (doubles): the unit's head (its multipliers' buffer holds lam_k, 8 per stage), then
constexpr int kValStride = 9;
constexpr int kValMat = 8 * kValStride;
constexpr int V_TR = B_END;                    // stage_AB's entries, 8 per stage: b00 b10 b20 E03 E04 E13 E14 E23
constexpr int V_D2 = V_TR + 8 * NS;            // T e33, T e44, T e34, T e03, T e04 of lam_{k+1}^T T f, 8 per stage
constexpr int V_PG = V_D2 + 8 * NS;            // P_{k+1}
constexpr int V_HH = V_PG + kValMat;           // G = P_{k+1} Acl_k
constexpr int V_AC = V_HH + kValMat;           // Acl_k, Acl_{k-1} (two buffers)
constexpr int V_KL = V_AC + 2 * kValMat;       // K_k, K_{k-1} (two buffers, rows r < 6)
constexpr int V_TOTAL = V_KL + 2 * kValMat;
static_assert(V_TOTAL * 8 <= 32 * 1024, "policy value kernel LDS");

// an entry of Acl_k = A_k + B_k K_k, the product rounded before the sum (nmpc_policy_covariance.hip's
// cov_acl: the same entry, bitwise)
__device__ __forceinline__ double val_acl(double a, double bik, double kij) {
#pragma clang fp contract(off)
  const double bk = bik * kij;
  return a + bk;
}

__global__ __launch_bounds__(WAVE) void nmpc_policy_value_kernel(const Params* __restrict__ prm, int B, int nc,
                                                                 ValIO io) {
  __shared__ __attribute__((aligned(16))) double smem[V_TOTAL];
  const int b = blockIdx.x;
  if (b >= B) return;
  Solver<CapEv> S{};
  LDS double* sm = (LDS double*)smem;
  GLB double* gw = (GLB double*)(io.ws + (long long)b * kProdWs);
  bind_solver(S, prm, sm, gw, b, kProdU, kProdGl, kProdHl, kProdTc, kProdDc);
  LDS double* tr = sm + V_TR;
  LDS double* d2 = sm + V_D2;
  LDS double* pg = sm + V_PG;
  LDS double* hh = sm + V_HH;
  const int N = S.N, nuE = S.nuE, nxE = prm->nxE, nn = nxE * nxE;
  const double T = S.T;
  const int lane = S.lanef();
  const int i = lane & 7, j = lane >> 3;
  const bool act = i < nxE && j < nxE;       // an entry of the nx x nx matrices
  const bool kact = i < nuE && j < nxE;      // an entry (r = i, j) of the nu x nx gain
  const int hi = i > j ? i : j, lo = i > j ? j : i;  // the lower-triangle entry this lane forms
  const int kr = i < 3 ? 0 : i - 2;          // row of K that row i of B_k K_k reads (B_k: column 0, then T)

  // ---------------- 1. scenario data; the plan into the solver's buffers
  load_params(S, prm, lane, io.p + (long long)b * io.ld_p);
  load_controls(S, prm, lane, io.ubar + (long long)b * io.ld_ubar, false);
  const double* Xb = io.Xbar + (long long)b * io.ld_Xbar;
  for (int q = lane; q < 8 * (N + 1); q += WAVE) {
    const int kk = q >> 3, c = q & 7;
    S.X[q] = c < nxE ? Xb[kk * nxE + c] : 0.0;  // (the no-gimbal model's absent states are 0)
  }
  for (int q = lane; q < 6 * kValMat; q += WAVE) pg[q] = 0.0;  // P, G, Acl x 2, K x 2
  if (lane < 8) S.lam[N * 8 + lane] = 0.0;                     // lam_N
  sync();
  // lane k: l_k; g_k, H_k and the trig cache (derivs synchronises); stage_AB's entries
  const double Jsum = wsum(lane < N ? S.stage_cost(S.X + lane * 8) : 0.0);
  S.derivs<true, false>(S.X, S.U);
  {
    const StageAB ab = point_stage_ab(S, lane);
    if (lane < N) {
      LDS double* t = tr + lane * 8;
      t[0] = ab.b00; t[1] = ab.b10; t[2] = ab.b20;
      t[3] = ab.E03; t[4] = ab.E04; t[5] = ab.E13; t[6] = ab.E14; t[7] = ab.E23;
    }
  }

  // stage k's global loads: this lane's own entry (r = i, j) of K_k, the entry its row of B_k K_k
  // reads, and its entry (hi, lo) of H_k (packed over the states a stage cost reads)
  const double* Kb = io.K ? io.K + (long long)b * io.ld_K : nullptr;
  const int vh = vloc(hi), vl = vloc(lo);
  const bool hact = act && vh >= 0 && vl >= 0;
  const int hq = hact ? hp(vl, vh) : 0;
  struct KLoad { double own, acl, h; };
  auto k_load = [&](int k, bool hess) {
    KLoad q{0.0, 0.0, 0.0};
    if (k < 0) return q;  // wave-uniform
    if (Kb) {
      const double* Kk = Kb + (long long)k * nuE * nxE;
      if (kact) q.own = Kk[j * nuE + i];
      if (act) q.acl = Kk[j * nuE + kr];
    }
    if (hess && hact) q.h = S.Hl[k * 21 + hq];
    return q;
  };
  // stage k's Acl_k and K_k into their LDS buffers
  auto stage_form = [&](int k, const KLoad& q) {
    if (k < 0) return;  // wave-uniform
    const LDS double* t = tr + k * 8;
    double a = i == j ? 1.0 : 0.0;
    if (i == 0 && j == 3) a = t[3];
    if (i == 0 && j == 4) a = t[4];
    if (i == 1 && j == 3) a = t[5];
    if (i == 1 && j == 4) a = t[6];
    if (i == 2 && j == 3) a = t[7];
    if (Kb) a = val_acl(a, i < 3 ? t[i] : T, q.acl);
    LDS double* ac = sm + V_AC + (k & 1) * kValMat;
    LDS double* kl = sm + V_KL + (k & 1) * kValMat;
    if (act) ac[i * kValStride + j] = a;
    if (kact) kl[i * kValStride + j] = q.own;
  };

  sync();  // (tr stands)
  // ---------------- 2. lam_k = g_k + Acl_k^T lam_{k+1}, lane i < 8 row i
  stage_form(N - 1, k_load(N - 1, false));
  sync();
  for (int k = N - 1; k >= 0; --k) {
    const KLoad kn = k_load(k - 1, false);
    const LDS double* ac = sm + V_AC + (k & 1) * kValMat;
    if (lane < 8) {
      double acc = i < nxE ? S.gl[k * 8 + i] : 0.0;
      const LDS double* ln = S.lam + (k + 1) * 8;
#pragma unroll
      for (int l = 0; l < 8; ++l) {
        if (l < nxE) acc = fma(ac[l * kValStride + i], ln[l], acc);
      }
      S.lam[k * 8 + i] = i < nxE ? acc : 0.0;
    }
    stage_form(k - 1, kn);
    sync();
  }

  // ---------------- 3. lane k: the dynamics' second-order terms at lam_{k+1}; lane (i, j): the
  // multipliers' outer products
  if (lane < N) {
    const Dyn2 e = point_dyn2(S, lane);
    LDS double* t = d2 + lane * 8;
    t[0] = T * e.e33; t[1] = T * e.e44; t[2] = T * e.e34; t[3] = T * e.e03; t[4] = T * e.e04;
  }
  const double l0i = S.lam[hi], l0j = S.lam[lo];
  double lsum = 0.0;
  for (int k = 1; k <= N; ++k) lsum = fma(S.lam[k * 8 + hi], S.lam[k * 8 + lo], lsum);
  if (io.lam) put_trajectory(prm, lane, S.lam, io.lam + (long long)b * (nxE * (N + 1)));

  // ---------------- 4. P_k = M_k + Acl_k^T P_{k+1} Acl_k
  double* Po = io.P ? io.P + (long long)b * nn * (N + 1) : nullptr;
  if (Po && act) Po[(long long)N * nn + j * nxE + i] = 0.0;  // P_N
  double pij = 0.0, psum = 0.0;
  KLoad kc = k_load(N - 1, true);
  stage_form(N - 1, kc);
  sync();  // (d2, Acl_{N-1}, K_{N-1} stand; P_N = 0 since the carve-up was cleared)
  for (int k = N - 1; k >= 0; --k) {
    const KLoad kn = k_load(k - 1, true);
    const LDS double* ac = sm + V_AC + (k & 1) * kValMat;
    const LDS double* kl = sm + V_KL + (k & 1) * kValMat;
    // G = P_{k+1} Acl_k: row i of P against column j of Acl
    double g = 0.0;
#pragma unroll
    for (int l = 0; l < 8; ++l) {
      if (l < nxE) g = fma(pg[i * kValStride + l], ac[l * kValStride + j], g);
    }
    hh[i * kValStride + j] = g;
    // M_k's entry (hi, lo), off the chain: Fxx has entries (3, 3), (4, 4), (4, 3); Fxu (3, u0), (4, u0)
    const LDS double* t = d2 + k * 8;
    const double fxx = lo == 3 ? (hi == 3 ? t[0] : (hi == 4 ? t[2] : 0.0)) : (lo == 4 && hi == 4 ? t[1] : 0.0);
    const double fh = hi == 3 ? t[3] : (hi == 4 ? t[4] : 0.0);
    const double fl = lo == 3 ? t[3] : (lo == 4 ? t[4] : 0.0);
    double mk = kc.h + fxx;
    if (Kb) {
      mk = fma(fh, kl[lo], mk);  // (Fxu K_k)[hi, lo]: row 0 of K_k is the speed's
      mk = fma(kl[hi], fl, mk);  // (K_k^T Fxu^T)[hi, lo]
    }
    sync();  // (G stands)
    double pn = mk;
#pragma unroll
    for (int l = 0; l < 8; ++l) {
      if (l < nxE) pn = fma(ac[l * kValStride + hi], hh[l * kValStride + lo], pn);
    }
    pij = act ? pn : 0.0;
    if (Po && act) Po[(long long)k * nn + j * nxE + i] = pij;
    if (k >= 1) psum = psum + pij;
    stage_form(k - 1, kn);
    kc = kn;
    pg[i * kValStride + j] = pij;
    sync();
  }

  // ---------------- 5. J; per case dJ and varJ from the lower triangles of S0 and W
  const bool bad = wany(lane < nxE && S.lam[lane] != S.lam[lane]);
  if (lane == 0 && io.J) io.J[b] = bad ? NAN : Jsum;
  if (!io.dJ && !io.varJ) return;  // wave-uniform
  const bool low = act && i >= j;
  const double cnt = i == j ? 1.0 : 2.0;
  for (int c = 0; c < nc; ++c) {
    double s = 0.0, w = 0.0;
    if (low) {
      s = io.S0[(long long)b * io.ld_S0 + (long long)c * nn + j * nxE + i];
      if (io.W) w = io.W[(long long)b * io.ld_W + (long long)c * nn + j * nxE + i];
    }
    // (a lane off the lower triangle contributes an exact 0, whatever its P and lam)
    const double dj = low ? cnt * fma(psum, w, pij * s) : 0.0;
    const double vj = low ? cnt * fma(lsum, w, (l0i * l0j) * s) : 0.0;
    const double djs = wsum(dj), vjs = wsum(vj);
    if (lane == 0) {
      if (io.dJ) io.dJ[(long long)b * nc + c] = 0.5 * djs;
      if (io.varJ) io.varJ[(long long)b * nc + c] = vjs;
    }
  }
}

}  // namespace

int nmpc_policy_value_launch(const Params* dprm, int B, int nc, const ValIO& io, void* stream) {
  hipLaunchKernelGGL(nmpc_policy_value_kernel, dim3(B), dim3(WAVE), 0, (hipStream_t)stream, dprm, B, nc, io);
  return (int)hipGetLastError();
}
