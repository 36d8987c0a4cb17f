// nmpc_policy_rollout.hip -- batched disturbance rollouts of the plan's feedback policy
// (nmpc_policy_rollout_batch / nmpc_policy_rollout_batch_dev, include/nmpc_amd.h): for each of B
// scenarios and each of M disturbance samples the clamped policy on the nonlinear plant,
//   x_0 = p[x0 block] + e0[s]
//   k = 0 ... N-1:  u_raw = ubar_k + K_k (x_k - Xbar_k)          (K null: open-loop replay of ubar)
//                   u_k   = min(max(u_raw, lbx_k), ubx_k)        (either bound null: not applied)
//                   J    += stage_cost(x_k; p)
//                   x_{k+1} = x_k + T f(x_k, u_k) + w_k[s]       (w null: no process disturbance)
// with its cost sum J, the worst violation of the rows g(x_0 ... x_N) against lbg, ubg, the number
// of control entries the clamp changed, and on request the trajectories.
//
// Part of the evaluation kernel's translation unit (nmpc_eval.hip includes this file last): the
// stage cost and the rows are Solver::stage_cost and Solver::row_value, the solver's own text,
// called on a pointer to the sample's current state; the dynamics are the operations of
// Solver::rollout in the sequential recursion's order, each product rounded before its sum (no
// contraction), so an undisturbed, unclamped sample reproduces Solver::rollout's X.
//
// Execution model: unlike every sibling, lane = sample.  One wavefront per (scenario, block of 64
// samples) on a grid of B x ceil(M / 64); the 64 lanes share the scenario's p, obstacle table,
// weights and Xbar (LDS, loaded as the evaluation kernel loads them) and read K_k, ubar_k and the
// bounds at wave-uniform addresses, while each lane carries its own state through the N stages.
// That state sits in an LDS slot of the lane's own, kRollStride = 9 doubles apart: with 18 dwords
// between neighbouring lanes the 32 lanes of a ds_read_b64 group fall on 32 distinct even banks
// of the 64, and the 16 lanes of a ds_write_b64 group on 16 distinct even banks of the 32 (a
// stride of 8 would put lanes l and l + 4 on one bank: 8-way and 4-way conflicts).  No lane reads
// another's slot, so the stage loop needs no synchronisation after the scenario data stand.
// Control flow is wave-uniform: lanes past M recompute sample M - 1 and store nothing.  Every
// per-state and per-control loop is unrolled over the layout's 8 and 6 with wave-uniform guards
// (no dynamically indexed private array); plain C++ stores only.
// A NaN among a sample's states, controls, row values or the bounds it meets makes its J and its
// viol NaN (the row maximum alone, fmax, would drop it); other samples are untouched.
// (included by nmpc_eval.hip)

namespace {

// LDS carve-up (doubles)
constexpr int kRollStride = 9;
constexpr int PR_PP = 0;                        // p, internal layout (<= 64)
constexpr int PR_OB = PR_PP + 64;                // obstacle x (16), y (16)
constexpr int PR_RV = PR_OB + 2 * NMPC_MAX_OBS;  // Solver::rvars; [30], [31] = cost weights
constexpr int PR_XB = PR_RV + 32;                // Xbar, 8 per stage
constexpr int PR_XL = PR_XB + 8 * kEvalStages;   // the lanes' states, kRollStride apart
constexpr int PR_TOTAL = PR_XL + kRollStride * WAVE;
static_assert(PR_TOTAL * 8 <= 16 * 1024, "policy rollout kernel LDS");

// x_{k+1} = x_k + T f(x_k, u_k) [+ w_k]: Solver::rollout's increments T u_{1+c}, T (v cp ct),
// T (v sp ct), T (v st), each rounded on its own and then added, as the recursion stores and sums them
__device__ __forceinline__ void roll_step(double (&x)[8], const double (&u)[6], double T) {
#pragma clang fp contract(off)
  const double ct = cos(x[3]), st = sin(x[3]), cp = cos(x[4]), sp = sin(x[4]);
  const double v = u[0];
  const double i0 = T * (v * cp * ct), i1 = T * (v * sp * ct), i2 = T * (v * st);
  x[0] = x[0] + i0;
  x[1] = x[1] + i1;
  x[2] = x[2] + i2;
#pragma unroll
  for (int c = 0; c < 5; ++c) {
    const double ic = T * u[1 + c];
    x[3 + c] = x[3 + c] + ic;
  }
}

__global__ __launch_bounds__(WAVE) void nmpc_policy_rollout_kernel(const Params* __restrict__ prm, int B, int M,
                                                                   RollIO io) {
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
  const int N = S.N, m = S.m, nuE = S.nuE, nwE = S.nwE, nxE = prm->nxE, nXE = nxE * (N + 1);
  const double T = S.T;
  const int lane = S.lanef();
  const long long s = (long long)blockIdx.y * WAVE + lane;
  const bool live = s < M;
  const long long sc = live ? s : M - 1;    // lanes past M recompute the last sample
  const long long col = (long long)b * M + sc;  // the sample's column of every output

  // ---------------- scenario data (the parameter half of nmpc_eval_shared.hip without the phase
  // timers' slots, which this carve-up does not have), and Xbar
  load_p(S, prm, lane, io.p + (long long)b * io.ld_p);
  sync();
  load_obstacles(S, prm, lane);
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
  const double* lgb = io.lbg ? io.lbg + (long long)b * io.ld_lbg : nullptr;
  const double* ugb = io.ubg ? io.ubg + (long long)b * io.ld_ubg : nullptr;
  // per-lane bases
  const double* e0 = io.e0 + (long long)b * io.ld_e0 + sc * nxE;
  const double* wl = io.w ? io.w + (long long)b * io.ld_w + sc * N * nxE : nullptr;
  double* Xo = io.X ? io.X + col * nXE : nullptr;
  double* Uo = io.U ? io.U + col * nwE : nullptr;

  // ---------------- x_0 = p[x0 block] + e0 (an absent gimbal state stays p's 0)
  LDS double* xl = sm + PR_XL + lane * kRollStride;
  double x[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    x[c] = S.pp[c];
    if (c < nxE) x[c] = x[c] + e0[c];
    xl[c] = x[c];
  }

  double J = 0.0, vmax = 0.0;
  bool bad = false;
  int nsat = 0;
  // stage k's rows at the state in the lane's slot, and the state out
  auto stage_out = [&](int k) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      bad |= x[c] != x[c];
      if (Xo && live && c < nxE) Xo[k * nxE + c] = x[c];
    }
    if (!io.viol) return;  // wave-uniform
    for (int i = 0; i < m; ++i) {
      const double g = S.row_value(xl, i);
      bad |= g != g;
      if (lgb) {
        const double lo = lgb[k * m + i], hi = ugb[k * m + i];
        if (hi < BIGB) vmax = fmax(vmax, g - hi);
        if (lo > -BIGB) vmax = fmax(vmax, lo - g);
        bad |= lo != lo || hi != hi;  // a NaN bound is neither present nor absent
      }
    }
  };

  for (int k = 0; k < N; ++k) {
    stage_out(k);
    // ---------------- the clamped policy's control
    double u[6];
    const double* Kk = Kb ? Kb + (long long)k * nuE * nxE : nullptr;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      u[r] = 0.0;
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
        if (Uo && live) Uo[k * nuE + r] = uc;
        u[r] = uc;
      }
    }
    J += S.stage_cost(xl);
    // ---------------- the plant
    roll_step(x, u, T);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (wl && c < nxE) x[c] = x[c] + wl[k * nxE + c];
      xl[c] = x[c];
    }
  }
  stage_out(N);
  if (!live) return;
  if (io.J) io.J[col] = bad ? NAN : J;
  if (io.viol) io.viol[col] = bad ? NAN : vmax;
  if (io.nsat) io.nsat[col] = nsat;
}

}  // namespace

int nmpc_policy_rollout_launch(const Params* dprm, int B, int M, const RollIO& io, void* stream) {
  hipLaunchKernelGGL(nmpc_policy_rollout_kernel, dim3(B, (M + WAVE - 1) / WAVE), dim3(WAVE), 0, (hipStream_t)stream,
                     dprm, B, M, io);
  return (int)hipGetLastError();
}
