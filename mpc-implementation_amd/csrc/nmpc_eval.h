// nmpc_eval.h -- what the host translation unit (the C-ABI in nmpc_solve.hip) and the
// evaluation kernel's translation unit (nmpc_eval.hip) share: the kernel's argument block,
// its slice of the handle's per-scenario workspace, and the launcher.  Included by both after
// nmpc_impl::Params is defined; none of the solver's class translation units sees it.
#ifndef NMPC_EVAL_H
#define NMPC_EVAL_H

namespace nmpc_impl {

// DEVICE pointers, layouts and leading dimensions as nmpc_eval_batch_dev (include/nmpc_amd.h);
// x and p are required, every other pointer may be null
struct EvalIO {
  const double *x, *p, *lam_g, *lam_x, *lbx, *ubx, *lbg, *ubg;
  long long ld_x, ld_p, ld_lam_g, ld_lam_x, ld_lbx, ld_ubx, ld_lbg, ld_ubg;
  double *f, *g, *X, *grad_f, *grad_l, *kkt;
  double* ws;  // B x kEvalWs doubles of the handle's workspace
};

// Per-scenario workspace (doubles), sized for N = NMPC_MAX_N and 5 + NMPC_MAX_OBS rows per
// stage: the controls in the kernel's 6-per-stage layout, the stage-cost gradients, the
// transcendental cache of the rollout and stage costs (12 per stage) and the row scaling
// (ones) the solver's adjoint multiplies by.  Every solver class's own workspace is larger
// (static_assert in nmpc_eval.hip), so a handle whose workspace covers B for a solve covers
// B for an evaluation.
constexpr int kEvalStages = NMPC_MAX_N + 1;
constexpr int kEvalU = 0;
constexpr int kEvalGl = kEvalU + 6 * kEvalStages;
constexpr int kEvalTc = kEvalGl + 8 * kEvalStages;
constexpr int kEvalDc = kEvalTc + 12 * kEvalStages;
constexpr int kEvalWs = kEvalDc + (5 + NMPC_MAX_OBS) * kEvalStages;

}  // namespace nmpc_impl

// Enqueues the evaluation of B scenarios on `stream` (one wavefront per scenario); returns
// the hipError_t of the launch.  No allocation, no synchronisation.
int nmpc_eval_launch(const nmpc_impl::Params* dprm, int B, const nmpc_impl::EvalIO& io, void* stream);

#endif  // NMPC_EVAL_H
