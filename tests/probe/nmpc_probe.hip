// nmpc_probe.hip -- test-side probes of the solver's device primitives.
//
// Includes the product's kernel source itself (NMPC_TU_CLASS == 0: no class kernel, no
// C-ABI), so wsum / wmax / wmin, readlane_d, LogAcc, rcp, rsq and qd below are the text the
// solver compiles, under the same flags (tests/probe/build.py).  Each probe kernel runs one
// 64-lane wave per workgroup, as the product's kernels do; the extern "C" launchers take
// host arrays and do their own device allocation and copies (no torch).  The product library
// never links or loads this file.
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
  void* p[8] = {};
  int np = 0;
  hipError_t err = hipSuccess;
  void* in(const void* host, size_t bytes) {
    void* d = out(bytes);
    if (d && err == hipSuccess) err = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
    return d;
  }
  void* out(size_t bytes) {
    void* d = nullptr;
    if (err == hipSuccess && np >= 8) err = hipErrorOutOfMemory;  // table full
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
