// dpenv_policy_xws2.hip - the two-wave closed-loop rollout, DPENV_POLICY_F32_ACTOR: actor in the split-f16 arithmetic, critic in plain f16
// (policy_rollout_ws_kernel<.., PREC_F32_ACTOR, GROUPS> of dpenv_policy_ws.h; arithmetic: mlp_eval_x in dpenv_policy_dev.h).
// Reference: rollout loop spinup/algos/tf1/ppo/ppo.py:289-322, fp32 networks core.py:29-33,80-107.
#include "dpenv_policy_ws.h"

namespace dpenv {
template hipError_t dev::launch_policy_rollout_ws<PREC_F32_ACTOR>(const StepArgs*, const PolicyArgs*, const IntegArgs*, const FilterArgs*, int, int,
                                                                    hipStream_t);
}
