// dpenv_policy_ws.hip - the two-wave closed-loop rollout in the f16 network arithmetic (DPENV_POLICY_F16 + DPENV_LAUNCH_TWO_WAVE):
// policy_rollout_ws_kernel<.., PREC_F16, GROUPS> of dpenv_policy_ws.h.  Its own translation unit: the instantiations take minutes.
// Reference: rollout loop spinup/algos/tf1/ppo/ppo.py:289-322, networks core.py:29-33,80-107.
#include "dpenv_policy_ws.h"

namespace dpenv {
template hipError_t dev::launch_policy_rollout_ws<PREC_F16>(const StepArgs*, const PolicyArgs*, const IntegArgs*, const FilterArgs*, int, int,
                                                                    hipStream_t);
}
