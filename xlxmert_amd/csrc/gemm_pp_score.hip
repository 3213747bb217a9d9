// XL_EPI_ROWSCORE instance of the ping-pong kernel: the head contraction of a forward-only validation pass, whose epilogue leaves
// per row and 64-column segment {max, sum exp, argmax, the label's logit} instead of logits (gemm_common.h epilogue_rows_fast) --
// the forward half of a fused logits + online log-sum-exp cross-entropy.  Forward layout, 256x256 tiles, every tile interior.
// A translation unit of its own: the other instances' objects do not change with it.
#include "gemm_pp_kernel.h"

namespace xl {

hipError_t launch_pp_score(const GemmParams& p, int nblk, hipStream_t st) {
    return launch_pp_one<true, true, XL_EPI_ROWSCORE, 256, 256>(p, nblk, st);
}

}  // namespace xl
