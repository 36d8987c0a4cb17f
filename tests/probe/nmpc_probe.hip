// nmpc_probe.hip -- test-side probes of the solver's device primitives.
//
// Includes the product's kernel source itself (NMPC_TU_CLASS == 0: no class kernel, no
// C-ABI), so wsum / wmax / wmin, readlane_d, LogAcc, rcp, rsq and qd below are the text the
// solver compiles, under the same flags (tests/probe/build.py); probe_lq_kernel further down
// runs the solver's factorisation, solves and fp64 refinement at a given point for one kernel
// class (fp64 or fp32 factors).  Each probe kernel runs one 64-lane wave per workgroup, as the
// product's kernels do; the extern "C" launchers take host arrays and do their own device
// allocation and copies (no torch).  The product library never links or loads this file.
#define NMPC_TU_CLASS 0
#include "../../mpc-implementation_amd/csrc/nmpc_solve.hip"

namespace {

// out[c * 64 + l] = the all-reduce of in[c * 64 + 0..63] as lane l holds it
__global__ __launch_bounds__(64) void probe_wreduce_kernel(int op, const double* in, double* out) {
  const long long i = (long long)blockIdx.x * WAVE + threadIdx.x;
  const double v = in[i];
  out[i] = op == 0 ? wsum(v) : (op == 1 ? wmax(v) : wmin(v));
}

// out[c * 64 + l] = lane src[c]'s value of in[c * 64 + 0..63], read by lane l
template <class T>
__global__ __launch_bounds__(64) void probe_readlane_kernel(const T* in, const int* src, T* out) {
  const long long i = (long long)blockIdx.x * WAVE + threadIdx.x;
  const int l = __builtin_amdgcn_readfirstlane(src[blockIdx.x]) & (WAVE - 1);
  out[i] = readlane_d(in[i], l);
}

// lane i: cnt[i] factors x[i * nf + 0..], through mul (pairs == 0) or mul2 (pairs == 1: the
// factors two at a time, an odd last one with 1.0 as the solver pads a missing bound)
__global__ __launch_bounds__(64) void probe_logacc_kernel(int pairs, int n, int nf, const double* x, const int* cnt,
                                                          double* out) {
  const long long i = (long long)blockIdx.x * WAVE + threadIdx.x;
  if (i >= n) return;
  const double* xi = x + i * nf;
  int c = cnt[i];
  c = c < 0 ? 0 : (c > nf ? nf : c);
  LogAcc la;
  if (pairs) {
    for (int j = 0; j < c; j += 2) la.mul2(xi[j], j + 1 < c ? xi[j + 1] : 1.0);
  } else {
    for (int j = 0; j < c; ++j) la.mul(xi[j]);
  }
  out[i] = la.log();
}

__global__ __launch_bounds__(64) void probe_unary_kernel(int op, long long n, const double* x, double* out) {
  const long long i = (long long)blockIdx.x * WAVE + threadIdx.x;
  if (i >= n) return;
  out[i] = op == 0 ? rcp(x[i]) : rsq(x[i]);
}

__global__ __launch_bounds__(64) void probe_rsqf_kernel(long long n, const float* x, float* out) {
  const long long i = (long long)blockIdx.x * WAVE + threadIdx.x;
  if (i >= n) return;
  out[i] = rsq(x[i]);
}

__global__ __launch_bounds__(64) void probe_qd_kernel(long long n, const double* a, const double* b, double* q) {
  const long long i = (long long)blockIdx.x * WAVE + threadIdx.x;
  if (i >= n) return;
  q[i] = qd(a[i], b[i]);
}

// device copies of host arrays, freed on scope exit; err holds the first HIP failure
struct Bufs {
  void* p[16] = {};
  int np = 0;
  hipError_t err = hipSuccess;
  void* in(const void* host, size_t bytes) {
    void* d = out(bytes);
    if (d && err == hipSuccess) err = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
    return d;
  }
  void* out(size_t bytes) {
    void* d = nullptr;
    if (err == hipSuccess && np >= 16) err = hipErrorOutOfMemory;  // table full
    if (err == hipSuccess) err = hipMalloc(&d, bytes ? bytes : 8);
    if (err != hipSuccess) return nullptr;
    p[np++] = d;
    return d;
  }
  void back(void* host, const void* dev, size_t bytes) {
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err == hipSuccess) err = hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost);
  }
  ~Bufs() {
    for (int i = 0; i < np; ++i) hipFree(p[i]);
  }
};
inline unsigned waves(long long n) { return (unsigned)((n + WAVE - 1) / WAVE); }

// ---- riccati -> resolve -> forward -> refine -> refine of one kernel class at a given point
//
// The inputs of nmpc_kkt_solve_batch (dense, one row per scenario): M dw = r_w + J^T r_g with
// M = W + diag(sigma_x) + delta I + J^T diag(sigma_s + delta) J.  The scenario is set up as
// nmpc_kkt_kernel sets it up (nmpc_kkt.hip steps 1-6: the stage summaries Qs / qs from the same
// expressions), but on Solver<CAP>::bind, so every buffer the class's riccati_ / resolve /
// forward / refine touch (rres, dUr, rdX, Xt, inc, the RowT rows) lies where the class's own
// kernels keep it: in the class's LDS carve-up CAP::L or its global workspace slice.  The gate
// of the restated setup is the test's independent dense matrix.
struct LqIO {
  const double *x, *p, *lam_g, *sigma_x, *sigma_s, *delta, *r_w, *r_g;
  double obj_factor;
  int nr;
  double *dw, *dX;  // [3][B][nr][nwE], [3][B][nr][nXE]: before, after one, after two refinements
  double* du;       // [3][B][nr][6 N]: the same steps in the kernel's layout, absent controls included
  int* info;        // 0, 1 (a pivot not positive), -11 (an invalid weight)
  double* ws;       // B x CAP::L.wstotal, zeroed
};

static_assert(CapA32::L.total * 8 <= 40960, "the LDS-row fp32 class's carve-up exceeds a quarter CU");
static_assert(CapC::L.total * 8 <= 65536 && CapC32::L.total * 8 <= 65536, "static LDS of the probe kernel");

template <class CAP>
__global__ __launch_bounds__(WAVE) void probe_lq_kernel(const Params* __restrict__ prm, int B, LqIO io) {
  __shared__ __attribute__((aligned(16))) double smem[CAP::L.total];
  const int b = blockIdx.x;
  if (b >= B) return;
  Solver<CAP> S;
  S.bind(prm, smem, io.ws, threadIdx.x, b);
  S.df = 1.0; S.mu = 0.0; S.tau = 0.0; S.nfilt = 0; S.nzx = 0; S.nzs = 0; S.rho = 0.0; S.etaR = 0.0;
  const int N = S.N, m = S.m, nb = S.nb, nw = S.nw, ng = S.ng, nwE = S.nwE, nuE = S.nuE;
  const int nxE = prm->nxE, nXE = nxE * (N + 1), nr = io.nr;
  const double T = S.T;
  const int lane = S.lanef();
  const double* yb = io.lam_g + (long long)b * ng;
  const double* xb = io.x + (long long)b * nwE;
  const double* sxb = io.sigma_x + (long long)b * nwE;
  const double* ssb = io.sigma_s + (long long)b * ng;
  const double* rwb = io.r_w + (long long)b * nr * nwE;
  const double* rgb = io.r_g + (long long)b * nr * ng;
  const double delta = io.delta[b];
  S.delta = delta;
  GLB double* Rd = S.sigx;  // sigma_x, the kernel's layout
  GLB double* rv = S.ru;    // the right-hand side's control terms
  const long long sw = (long long)B * nr * nwE, sX = (long long)B * nr * nXE;

  auto finish_nan = [&](int verdict) {
    for (int t = 0; t < 3; ++t) {
      for (long long i = lane; i < (long long)nr * nwE; i += WAVE) io.dw[t * sw + (long long)b * nr * nwE + i] = NAN;
      for (long long i = lane; i < (long long)nr * nXE; i += WAVE) io.dX[t * sX + (long long)b * nr * nXE + i] = NAN;
      for (long long i = lane; i < (long long)nr * nw; i += WAVE) io.du[((long long)t * B + b) * nr * nw + i] = NAN;
    }
    if (lane == 0) io.info[b] = verdict;
  };

  // scenario data
  for (int i = lane; i < prm->np; i += WAVE) {
    const int e = ext_p(prm, i);
    S.pp[i] = e >= 0 ? io.p[(long long)b * prm->npE + e] : 0.0;
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

  // the weights
  bool bad = !(delta >= 0.0) || delta == INFINITY;
  int fmk = 0;
  if (lane < N) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const double v = c < nuE ? sxb[lane * nuE + c] : 0.0;
      const bool fx = v == INFINITY;
      bad |= !(v >= 0.0);
      fmk |= fx ? (1 << c) : 0;
      Rd[lane * 6 + c] = fx ? 0.0 : v;
      rv[lane * 6 + c] = 0.0;
    }
  }
  if (lane <= N) S.fixm[lane] = fmk;
  for (int r = m + lane; r < ng; r += WAVE) {
    const double v = ssb[r];
    bad |= !(v >= 0.0) || v == INFINITY;
  }
  S.nfix = wany(fmk != 0) ? 1 : 0;
  if (wany(bad)) {
    finish_nan(-11);
    return;
  }
  sync();

  // rollout, stage costs (their transcendentals), derivatives, multipliers
  S.rollout(S.U, S.X);
  if (lane < N) (void)S.stage_cost(S.X + lane * 8, S.tc + lane * 12);
  sync();
  S.template derivs<true, true>(S.X, S.U, S.tc);
  S.adjoint(io.obj_factor, yb);

  // lane k: the stage summary (nmpc_kkt.hip step 4)
  const int k = lane;
  if (k <= N) {
    double Q[36];
#pragma unroll
    for (int t = 0; t < 36; ++t) Q[t] = 0.0;
    double s03 = 0.0, s04 = 0.0;
    if (k >= 1) {
      const LDS double* xk = S.X + k * 8;
      double Qxy0 = 0, Qxy1 = 0, Qxy2 = 0;
      double Qb[5] = {0, 0, 0, 0, 0};
      for (int i = 0; i < m; ++i) {
        const int r = k * m + i;
        const double w = ssb[r] + delta;
        if (i < nb) {
          Qb[i] = w;
        } else {
          const double C = yb[r];
          const int o = i - nb;
          const double ddx = xk[0] - S.obx[o], ddy = xk[1] - S.oby[o];
          const double idd = rsq(ddx * ddx + ddy * ddy);
          const double gx = -(ddx * idd), gy = -(ddy * idd);
          const double id3 = idd * idd * idd;
          Qxy0 += w * gx * gx + C * (-ddy * ddy * id3);
          Qxy1 += w * gx * gy + C * (ddx * ddy * id3);
          Qxy2 += w * gy * gy + C * (-ddx * ddx * id3);
        }
      }
      const int sv[6] = {0, 1, 2, 5, 6, 7};
#pragma unroll
      for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int bq = a; bq < 6; ++bq) Q[S.pk8(sv[a], sv[bq])] += io.obj_factor * S.Hl[k * 21 + hp(a, bq)];
      }
      Q[S.pk8(0, 0)] += Qxy0; Q[S.pk8(0, 1)] += Qxy1; Q[S.pk8(1, 1)] += Qxy2;
      Q[S.pk8(2, 2)] += Qb[0]; Q[S.pk8(3, 3)] += Qb[1]; Q[S.pk8(5, 5)] += Qb[2];
      Q[S.pk8(6, 6)] += Qb[3]; Q[S.pk8(7, 7)] += Qb[4];
      if (k < N) {
        const LDS double* tg = S.trig + k * 8;
        const double ct = tg[0], stt = tg[1], cp = tg[2], sp = tg[3], v = tg[4];
        const LDS double* ln = S.lam + (k + 1) * 8;
        const double l0 = ln[0], l1 = ln[1], l2 = ln[2];
        Q[S.pk8(3, 3)] += T * (-l0 * v * cp * ct - l1 * v * sp * ct - l2 * v * stt);
        Q[S.pk8(4, 4)] += T * (-l0 * v * cp * ct - l1 * v * sp * ct);
        Q[S.pk8(3, 4)] += T * (l0 * v * sp * stt - l1 * v * cp * stt);
        s03 = T * (-l0 * cp * stt - l1 * sp * stt + l2 * ct);
        s04 = T * (-l0 * sp * ct + l1 * cp * ct);
      }
    }
#pragma unroll
    for (int t = 0; t < 36; ++t) S.Qs[k * 36 + t] = Q[t];
    LDS double* qo = S.qs + k * 10;
#pragma unroll
    for (int c = 0; c < 8; ++c) qo[c] = 0.0;
    qo[8] = s03;
    qo[9] = s04;
  }
  sync();

  // factorisation and inertia (zero linear terms)
  if (!S.riccati(Rd, rv)) {
    finish_nan(1);
    return;
  }
  sync();
  if (lane == 0) io.info[b] = 0;

  // the step as the class holds it (no masking here: a fixed or absent control's entry is what
  // forward / refine left there)
  auto store = [&](int t, int d) {
    double* ow = io.dw + t * sw + ((long long)b * nr + d) * nwE;
    for (int i = lane; i < nw; i += WAVE) {
      const int e = ext_u(prm, i);
      if (e >= 0) ow[e] = S.dU[i];
      io.du[(((long long)t * B + b) * nr + d) * nw + i] = S.dU[i];
    }
    double* oX = io.dX + t * sX + ((long long)b * nr + d) * nXE;
    for (int i = lane; i < prm->nX; i += WAVE) {
      const int kk = i >> 3, c = i & 7;
      if (c < nxE) oX[kk * nxE + c] = S.dX[i];
    }
    sync();
  };

  for (int d = 0; d < nr; ++d) {
    // r_k = -r_w, q_k = -G_k^T r_g (nmpc_kkt.hip step 6)
    for (int i = lane; i < nw; i += WAVE) {
      const int e = ext_u(prm, i);
      rv[i] = e >= 0 ? -rwb[(long long)d * nwE + e] : 0.0;
    }
    if (k >= 1 && k <= N) {
      const LDS double* xk = S.X + k * 8;
      double q8[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) q8[c] = 0.0;
      const double* rg = rgb + (long long)d * ng;
      double qx = 0.0, qy = 0.0;
      for (int i = 0; i < m; ++i) {
        const double t = -rg[k * m + i];
        if (i < nb) {
          const int bi = boxidx(i);
#pragma unroll
          for (int c = 2; c < 8; ++c) q8[c] = c == bi ? t : q8[c];
        } else {
          const int o = i - nb;
          const double ddx = xk[0] - S.obx[o], ddy = xk[1] - S.oby[o];
          const double idd = rsq(ddx * ddx + ddy * ddy);
          qx += t * (-(ddx * idd));
          qy += t * (-(ddy * idd));
        }
      }
      q8[0] = qx;
      q8[1] = qy;
      LDS double* qo = S.qs + k * 10;
#pragma unroll
      for (int c = 0; c < 8; ++c) qo[c] = q8[c];
    }
    sync();
    // the solver's calls after a factorisation, and one more refinement
    S.resolve(rv);
    S.forward(S.dU, S.dX);
    store(0, d);
    S.refine(Rd, rv, S.dU, S.dX);
    store(1, d);
    S.refine(Rd, rv, S.dU, S.dX);
    store(2, d);
  }
}

// nmpc_create's Params of a problem description (the host side of the solver is not part of
// this unit: NMPC_TU_CLASS 0); false: a shape nmpc_create refuses
inline bool params_of(const nmpc_desc* desc, Params& P) {
  if (desc->model != NMPC_MODEL_UAV8G && desc->model != NMPC_MODEL_UAV5) return false;
  const bool nog = desc->model == NMPC_MODEL_UAV5;
  if (desc->N < 1 || desc->N > NMPC_MAX_N || desc->n_obs < 0 || desc->n_obs > NMPC_MAX_OBS) return false;
  if (desc->np < (nog ? 8 : 11) || desc->np > 61 || !(desc->T > 0)) return false;
  auto pin = [&](int e) { return (e < 0 || !nog) ? e : e + 3; };
  std::memset(&P, 0, sizeof(P));
  P.model = desc->model;
  P.nb = nog ? 2 : 5;
  P.nuE = nog ? 3 : 6; P.nxE = nog ? 5 : 8;
  P.N = desc->N; P.nobs = desc->n_obs; P.m = P.nb + desc->n_obs;
  P.npE = desc->np; P.np = desc->np + (nog ? 3 : 0);
  P.nw = 6 * P.N; P.nwE = P.nuE * P.N; P.ng = P.m * (P.N + 1); P.nX = 8 * (P.N + 1);
  P.T = desc->T; P.w1 = desc->w1; P.w2 = nog ? 0.0 : desc->w2; P.hv = desc->vfov / 2; P.hh = desc->hfov / 2;
  P.thv = std::tan(P.hv); P.thh = std::tan(P.hh);
  P.w1p = pin(desc->w1_pidx); P.w2p = nog ? -1 : pin(desc->w2_pidx);
  for (int j = 0; j < NMPC_MAX_OBS; ++j) {
    P.oxp[j] = -1; P.oyp[j] = -1;
  }
  for (int j = 0; j < desc->n_obs; ++j) {
    if (desc->obs_x_pidx[j] >= desc->np || desc->obs_y_pidx[j] >= desc->np) return false;
    P.ox[j] = desc->obs_x[j]; P.oy[j] = desc->obs_y[j]; P.orr[j] = desc->obs_rsum[j];
    P.oxp[j] = pin(desc->obs_x_pidx[j]); P.oyp[j] = pin(desc->obs_y_pidx[j]);
  }
  if (desc->w1_pidx >= desc->np || desc->w2_pidx >= desc->np) return false;
  P.o = desc->opts;
  return true;
}

template <class CAP>
int lq_step(const Params& P, int B, int nr, LqIO io, double* dw, double* dX, double* du, int* info) {
  if (P.N > CAP::nmax || P.m > CAP::mmax) return (int)hipErrorInvalidValue;  // the class's capacity
  Bufs b;
  const size_t nwE = (size_t)P.nwE, ng = (size_t)P.ng, nXE = (size_t)P.nxE * (P.N + 1), D = sizeof(double);
  const Params* dprm = (const Params*)b.in(&P, sizeof(Params));
  io.x = (const double*)b.in(io.x, B * nwE * D);
  io.p = (const double*)b.in(io.p, (size_t)B * P.npE * D);
  io.lam_g = (const double*)b.in(io.lam_g, B * ng * D);
  io.sigma_x = (const double*)b.in(io.sigma_x, B * nwE * D);
  io.sigma_s = (const double*)b.in(io.sigma_s, B * ng * D);
  io.delta = (const double*)b.in(io.delta, B * D);
  io.r_w = (const double*)b.in(io.r_w, (size_t)B * nr * nwE * D);
  io.r_g = (const double*)b.in(io.r_g, (size_t)B * nr * ng * D);
  const size_t bw = 3 * (size_t)B * nr * nwE * D, bX = 3 * (size_t)B * nr * nXE * D, bws = (size_t)B * CAP::L.wstotal * D;
  io.dw = (double*)b.out(bw);
  io.dX = (double*)b.out(bX);
  const size_t bu = 3 * (size_t)B * nr * P.nw * D;
  io.du = (double*)b.out(bu);
  io.info = (int*)b.out((size_t)B * sizeof(int));
  io.ws = (double*)b.out(bws);
  if (b.err == hipSuccess) b.err = hipMemset(io.ws, 0, bws);
  if (b.err == hipSuccess) b.err = hipMemset(io.info, 0xFF, (size_t)B * sizeof(int));
  if (b.err != hipSuccess) return (int)b.err;
  hipLaunchKernelGGL(probe_lq_kernel<CAP>, dim3(B), dim3(WAVE), 0, 0, dprm, B, io);
  b.back(dw, io.dw, bw);
  if (b.err == hipSuccess) b.err = hipMemcpy(dX, io.dX, bX, hipMemcpyDeviceToHost);
  if (b.err == hipSuccess) b.err = hipMemcpy(du, io.du, bu, hipMemcpyDeviceToHost);
  if (b.err == hipSuccess) b.err = hipMemcpy(info, io.info, (size_t)B * sizeof(int), hipMemcpyDeviceToHost);
  return (int)b.err;
}

}  // namespace

extern "C" {

// every launcher returns 0 or the hipError_t of the first failure

// op 0 / 1 / 2: wsum / wmax / wmin over ncase waves of 64 values
int nmpc_probe_wreduce(int op, int ncase, const double* in, double* out) {
  if (ncase <= 0 || op < 0 || op > 2 || !in || !out) return (int)hipErrorInvalidValue;
  Bufs b;
  const size_t bytes = (size_t)ncase * WAVE * sizeof(double);
  const double* din = (const double*)b.in(in, bytes);
  double* dout = (double*)b.out(bytes);
  if (b.err != hipSuccess) return (int)b.err;
  hipLaunchKernelGGL(probe_wreduce_kernel, dim3(ncase), dim3(WAVE), 0, 0, op, din, dout);
  b.back(out, dout, bytes);
  return (int)b.err;
}

int nmpc_probe_readlane_f64(int ncase, const double* in, const int* src, double* out) {
  if (ncase <= 0 || !in || !src || !out) return (int)hipErrorInvalidValue;
  Bufs b;
  const size_t bytes = (size_t)ncase * WAVE * sizeof(double);
  const double* din = (const double*)b.in(in, bytes);
  const int* dsrc = (const int*)b.in(src, (size_t)ncase * sizeof(int));
  double* dout = (double*)b.out(bytes);
  if (b.err != hipSuccess) return (int)b.err;
  hipLaunchKernelGGL(probe_readlane_kernel<double>, dim3(ncase), dim3(WAVE), 0, 0, din, dsrc, dout);
  b.back(out, dout, bytes);
  return (int)b.err;
}

int nmpc_probe_readlane_f32(int ncase, const float* in, const int* src, float* out) {
  if (ncase <= 0 || !in || !src || !out) return (int)hipErrorInvalidValue;
  Bufs b;
  const size_t bytes = (size_t)ncase * WAVE * sizeof(float);
  const float* din = (const float*)b.in(in, bytes);
  const int* dsrc = (const int*)b.in(src, (size_t)ncase * sizeof(int));
  float* dout = (float*)b.out(bytes);
  if (b.err != hipSuccess) return (int)b.err;
  hipLaunchKernelGGL(probe_readlane_kernel<float>, dim3(ncase), dim3(WAVE), 0, 0, din, dsrc, dout);
  b.back(out, dout, bytes);
  return (int)b.err;
}

// n lanes, each with cnt[i] <= nf factors x[i * nf + j]; pairs: LogAcc::mul2, else LogAcc::mul
int nmpc_probe_logacc(int pairs, int n, int nf, const double* x, const int* cnt, double* out) {
  if (n <= 0 || nf <= 0 || !x || !cnt || !out) return (int)hipErrorInvalidValue;
  Bufs b;
  const double* dx = (const double*)b.in(x, (size_t)n * nf * sizeof(double));
  const int* dc = (const int*)b.in(cnt, (size_t)n * sizeof(int));
  double* dout = (double*)b.out((size_t)n * sizeof(double));
  if (b.err != hipSuccess) return (int)b.err;
  hipLaunchKernelGGL(probe_logacc_kernel, dim3(waves(n)), dim3(WAVE), 0, 0, pairs, n, nf, dx, dc, dout);
  b.back(out, dout, (size_t)n * sizeof(double));
  return (int)b.err;
}

// op 0 / 1: rcp / rsq (double)
int nmpc_probe_unary(int op, long long n, const double* x, double* out) {
  if (n <= 0 || op < 0 || op > 1 || !x || !out) return (int)hipErrorInvalidValue;
  Bufs b;
  const double* dx = (const double*)b.in(x, (size_t)n * sizeof(double));
  double* dout = (double*)b.out((size_t)n * sizeof(double));
  if (b.err != hipSuccess) return (int)b.err;
  hipLaunchKernelGGL(probe_unary_kernel, dim3(waves(n)), dim3(WAVE), 0, 0, op, n, dx, dout);
  b.back(out, dout, (size_t)n * sizeof(double));
  return (int)b.err;
}

int nmpc_probe_rsqf(long long n, const float* x, float* out) {
  if (n <= 0 || !x || !out) return (int)hipErrorInvalidValue;
  Bufs b;
  const float* dx = (const float*)b.in(x, (size_t)n * sizeof(float));
  float* dout = (float*)b.out((size_t)n * sizeof(float));
  if (b.err != hipSuccess) return (int)b.err;
  hipLaunchKernelGGL(probe_rsqf_kernel, dim3(waves(n)), dim3(WAVE), 0, 0, n, dx, dout);
  b.back(out, dout, (size_t)n * sizeof(float));
  return (int)b.err;
}

// cls 0 / 1 / 2: the fp64 global-row class (CapC), the fp32 global-row class (CapC32), the fp32
// LDS-row class (CapA32: N <= 20, m <= 15).  Dense inputs of nmpc_kkt_solve_batch, one row per
// scenario (x: B x nw, r_w: B x nr x nw, ...; sigma_x = +inf: fixed).  dw: 3 x B x nr x nw and
// dX: 3 x B x nr x nX -- the step after forward, after one and after two refinements; du: 3 x B
// x nr x 6 N, the same steps in the kernel's layout (six controls per stage); info: B.
int nmpc_probe_lq_step(int cls, const nmpc_desc* desc, int B, int nr, const double* x, const double* p,
                       const double* lam_g, double obj_factor, const double* sigma_x, const double* sigma_s,
                       const double* delta, const double* r_w, const double* r_g, double* dw, double* dX, double* du,
                       int* info) {
  if (!desc || B <= 0 || nr <= 0 || !x || !p || !lam_g || !sigma_x || !sigma_s || !delta || !r_w || !r_g || !dw ||
      !dX || !du || !info)
    return (int)hipErrorInvalidValue;
  Params P;
  if (!params_of(desc, P)) return (int)hipErrorInvalidValue;
  LqIO io{};
  io.x = x; io.p = p; io.lam_g = lam_g; io.sigma_x = sigma_x; io.sigma_s = sigma_s; io.delta = delta;
  io.r_w = r_w; io.r_g = r_g; io.obj_factor = obj_factor; io.nr = nr;
  switch (cls) {
    case 0: return lq_step<CapC>(P, B, nr, io, dw, dX, du, info);
    case 1: return lq_step<CapC32>(P, B, nr, io, dw, dX, du, info);
    case 2: return lq_step<CapA32>(P, B, nr, io, dw, dX, du, info);
    default: return (int)hipErrorInvalidValue;
  }
}

int nmpc_probe_qd(long long n, const double* a, const double* b_, double* q) {
  if (n <= 0 || !a || !b_ || !q) return (int)hipErrorInvalidValue;
  Bufs b;
  const double* da = (const double*)b.in(a, (size_t)n * sizeof(double));
  const double* db = (const double*)b.in(b_, (size_t)n * sizeof(double));
  double* dq = (double*)b.out((size_t)n * sizeof(double));
  if (b.err != hipSuccess) return (int)b.err;
  hipLaunchKernelGGL(probe_qd_kernel, dim3(waves(n)), dim3(WAVE), 0, 0, n, da, db, dq);
  b.back(q, dq, (size_t)n * sizeof(double));
  return (int)b.err;
}

}  // extern "C"
