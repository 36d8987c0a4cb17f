// nmpc_eval.hip -- batched evaluation of the NLP's function layer at GIVEN points
// (nmpc_eval_batch / nmpc_eval_batch_dev, include/nmpc_amd.h): for each of B scenarios
//   f(w, p), g(w, p), X(w, p), grad_w f, grad_w f + J_g^T lam_g + lam_x
// and the five numbers of a first-order (KKT) certificate.  CasADi's nlp_f / nlp_g /
// nlp_grad_f of the reference's nlpsol object, and ff(u, p) of Python/NMPC_TT.py:368.
//
// A translation unit of its own: it includes the solver's source with NMPC_TU_CLASS == 0 (no
// class kernel, no C-ABI), so the model is the text the solver compiles -- Solver::rollout,
// stage_cost, row_value, derivs, stage_AB, adjoint and grad_u -- while none of the solver's
// class translation units contains a line of this file.
//
// Execution model: the solver's.  One wavefront per scenario, stage k on lane k
// (N + 1 <= 64), decision variables and rows strided over the lanes, all control flow
// wave-uniform.
//   1. p, obstacle coordinates and cost weights to LDS; w to the workspace in the kernel's
//      6-controls-per-stage layout (the no-gimbal model's absent controls are 0);
//   2. rollout by per-lane in-order prefix sums (Solver::rollout);
//   3. lane k: stage cost l_k (k < N) and its rows g_{k,.}; f by the butterfly all-reduce;
//      with kkt_out the rows' violation, complementarity and multiplier size on the way;
//   4. stage-cost gradients (Solver::derivs, no Hessian) and the adjoint sweep
//      lam_k = grad l_k [+ G_k^T y_k] + A_k^T lam_{k+1} (Solver::adjoint: suffix sums, A_k only
//      couples the positions to theta, psi), grad_{u_k} = B_k^T lam_{k+1} (Solver::grad_u).
//      Once for the objective alone, once more with y = lam_g when lam_g is given.  Lane 0's
//      lam_0 is never read: stage 0 is constant in w, its terms are structurally absent;
//   5. decision variables: gradients out, stationarity / bound violation / complementarity.
// The certificate's maxima propagate NaN (fmax alone would drop it and certify a poisoned
// point).
#define NMPC_TU_CLASS 0
#include "nmpc_solve.hip"
#include "nmpc_eval.h"

namespace {

// the solver class whose code is instantiated here: any supported shape, global row vectors
// (so the adjoint's row scaling is read from the workspace, not from an LDS layout)
using CapEv = CapC;
static_assert(CapEv::nmax == NMPC_MAX_N && CapEv::mmax == 5 + NMPC_MAX_OBS && !CapEv::lds_rows,
              "the evaluation kernel instantiates the any-shape, global-row class");
static_assert(!Solver<CapEv>::kUnrollStages, "no -0.0 row in this kernel's stage scratch");

}  // namespace

// what the kernels of this unit share (no kernel of its own)
#include "nmpc_eval_shared.hip"

namespace {

static_assert(fits_every_class(kEvalWs), "a solver class's workspace is smaller than the evaluation's");

// LDS carve-up (doubles): the unit's head, then
constexpr int E_GF = B_END;                   // grad f, 6 per stage (internal layout)
constexpr int E_GL = E_GF + 6 * NS;           // grad of the Lagrangian
constexpr int E_TOTAL = E_GL + 6 * NS;
static_assert(E_TOTAL * 8 <= 32 * 1024, "evaluation kernel LDS");

// running maximum that remembers a NaN
struct MaxAcc {
  double v = 0.0;
  bool bad = false;
  __device__ __forceinline__ void add(double x) {
    bad |= x != x;
    v = fmax(v, x);
  }
  __device__ __forceinline__ double all() const {  // wave-uniform
    const double r = wmax(v);
    return wany(bad) ? NAN : r;
  }
};
// a value's bound violation and its multiplier's complementarity product (include/nmpc_amd.h)
__device__ __forceinline__ void kkt_terms(double v, double lam, double lo, double hi, MaxAcc& viol, MaxAcc& compl_,
                                          MaxAcc& lmax) {
  const bool hasl = lo > -BIGB, hasu = hi < BIGB;
  if (hasu) viol.add(v - hi);
  if (hasl) viol.add(lo - v);
  if (hi != hi || lo != lo) viol.bad = true;  // a NaN bound is neither present nor absent
  lmax.add(fabs(lam));
  if (lam > 0.0) compl_.add(hasu ? fabs(lam * (hi - v)) : 0.0);
  else if (lam < 0.0) compl_.add(hasl ? fabs(lam * (v - lo)) : 0.0);
  else if (lam != lam) compl_.bad = true;
}

__global__ __launch_bounds__(WAVE) void nmpc_eval_kernel(const Params* __restrict__ prm, int B, EvalIO io) {
  __shared__ __attribute__((aligned(16))) double smem[E_TOTAL];
  const int b = blockIdx.x;
  if (b >= B) return;
  Solver<CapEv> S{};
  LDS double* sm = (LDS double*)smem;
  GLB double* gw = (GLB double*)(io.ws + (long long)b * kEvalWs);
  // (Hl on gl: never written, derivs<false>)
  bind_solver(S, prm, sm, gw, b, kEvalU, kEvalGl, kEvalGl, kEvalTc, kEvalDc);
  LDS double* gF = sm + E_GF;
  LDS double* gL = sm + E_GL;
  const int N = S.N, m = S.m, nw = S.nw, ng = S.ng, nwE = S.nwE;
  const int lane = S.lanef();
  const bool want_grad = io.grad_f || io.grad_l || io.kkt;
  const double* yb = io.lam_g ? io.lam_g + (long long)b * io.ld_lam_g : nullptr;
  const double* lxb = io.lam_x ? io.lam_x + (long long)b * io.ld_lam_x : nullptr;
  const double* xb = io.x + (long long)b * io.ld_x;

  // ---------------- scenario data
  load_params(S, prm, lane, io.p + (long long)b * io.ld_p);
  load_controls(S, prm, lane, xb, want_grad && yb);
  sync();

  // ---------------- X, f, g
  S.rollout(S.U, S.X);
  MaxAcc viol, cpl, lmax;
  {
    const int k = lane;
    double f = 0.0;
    if (k <= N) {
      const LDS double* xk = S.X + k * 8;
      if (k < N) f = S.stage_cost(xk, S.tc + k * 12);
      for (int i = 0; i < m; ++i) {
        const int r = k * m + i;
        const double g = S.row_value(xk, i);
        if (io.g) io.g[(long long)b * ng + r] = g;
        if (io.kkt)
          kkt_terms(g, yb ? yb[r] : 0.0, io.lbg[(long long)b * io.ld_lbg + r], io.ubg[(long long)b * io.ld_ubg + r],
                    viol, cpl, lmax);
      }
    }
    const double fs = wsum(f);
    if (lane == 0 && io.f) io.f[b] = fs;
  }
  if (io.X) put_trajectory(prm, lane, S.X, io.X + (long long)b * (prm->nxE * (N + 1)));
  if (!want_grad) return;

  // ---------------- gradients: objective, then Lagrangian
  S.derivs<false, true>(S.X, S.U, S.tc);
  S.adjoint(1.0, (const double*)nullptr);
  for (int i = lane; i < nw; i += WAVE) gF[i] = S.grad_u(i);
  sync();
  if (yb) {
    S.adjoint(1.0, yb);
    for (int i = lane; i < nw; i += WAVE) gL[i] = S.grad_u(i);
  } else {
    for (int i = lane; i < nw; i += WAVE) gL[i] = gF[i];
  }
  MaxAcc stat, gmax;
  for (int i = lane; i < nw; i += WAVE) {
    const int e = ext_u(prm, i);
    if (e < 0) continue;
    const double lx = lxb ? lxb[e] : 0.0;
    const double gf = gF[i];
    const double gl_ = lxb ? gL[i] + lx : gL[i];
    if (io.grad_f) io.grad_f[(long long)b * nwE + e] = gf;
    if (io.grad_l) io.grad_l[(long long)b * nwE + e] = gl_;
    if (io.kkt) {
      stat.add(fabs(gl_));
      gmax.add(fabs(gf));
      kkt_terms(xb[e], lx, io.lbx[(long long)b * io.ld_lbx + e], io.ubx[(long long)b * io.ld_ubx + e], viol, cpl, lmax);
    }
  }
  if (io.kkt) {
    const double r0 = stat.all(), r1 = gmax.all(), r2 = viol.all(), r3 = cpl.all(), r4 = lmax.all();
    if (lane == 0) {
      double* kk = io.kkt + (long long)b * 5;
      kk[0] = r0; kk[1] = r1; kk[2] = r2; kk[3] = r3; kk[4] = r4;
    }
  }
}

}  // namespace

int nmpc_eval_launch(const Params* dprm, int B, const EvalIO& io, void* stream) {
  hipLaunchKernelGGL(nmpc_eval_kernel, dim3(B), dim3(WAVE), 0, (hipStream_t)stream, dprm, B, io);
  return (int)hipGetLastError();
}

// the Jacobian- and Hessian-vector products at given points: a second kernel of this unit
#include "nmpc_products.hip"

// the condensed KKT solves at given points: a third kernel of this unit
#include "nmpc_kkt.hip"

// the parameter-direction products at given points: a fourth kernel of this unit
#include "nmpc_pproducts.hip"

// the adjoint (transposed) products at given points: a fifth kernel of this unit
#include "nmpc_adjoint.hip"

// what the kernels at a solve's point share (no kernel of its own)
#include "nmpc_point.hip"

// the reverse-mode sensitivity of a solution in one launch: a sixth kernel of this unit
#include "nmpc_solve_adjoint.hip"

// the forward-mode sensitivity of a solution in one launch: a seventh kernel of this unit
#include "nmpc_solve_tangent.hip"

// the plan's feedback policy (stage gains and feedforward) in one launch: an eighth kernel of this unit
#include "nmpc_solve_policy.hip"

// disturbance rollouts of that policy on the plant, one lane per sample: a ninth kernel of this unit
#include "nmpc_policy_rollout.hip"

// the reverse sweep of those rollouts, one lane per sample again: a tenth kernel of this unit
#include "nmpc_policy_rollout_adjoint.hip"

// the cost-to-go expansion of that policy (expected cost and its variance), one wavefront per
// scenario: a thirteenth kernel of this unit
#include "nmpc_policy_value.hip"

// the closed-loop covariance of that policy and its rows' standard deviations, one wavefront per
// (scenario, case): an eleventh kernel of this unit
#include "nmpc_policy_covariance.hip"
