// XL_EPI_ROWSAMPLE instance of the ping-pong kernel: the codebook contraction of the temperature samplers, whose epilogue leaves
// per row and 64-column segment {max, sum exp, Gumbel-max draw, its logit} instead of logits (gemm_common.h epilogue_rows_fast).
// Forward layout, 256x256 tiles, every tile interior.  A translation unit of its own: the other instances' objects do not change
// with it.
#include "gemm_pp_kernel.h"

namespace xl {

hipError_t launch_pp_sample(const GemmParams& p, int nblk, hipStream_t st) {
    return launch_pp_one<true, true, XL_EPI_ROWSAMPLE, 256, 256>(p, nblk, st);
}

}  // namespace xl
