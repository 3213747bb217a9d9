// XL_EPI_RESIDUAL_F32 instances of the ping-pong kernel: the residual epilogue of the fp32 residual stream (fp32 operand and
// output beside bf16 A / B), forward and dX layouts, 256x256 tiles and the 128x192 "duo" tiles of the language stream.  A
// translation unit of its own: the other instances' objects do not change with it.
#include "gemm_pp_kernel.h"

namespace xl {

hipError_t launch_pp_res32(const GemmParams& p, int b_kmajor, int bm, int nblk, hipStream_t st) {
    constexpr int E = XL_EPI_RESIDUAL_F32;
    if (bm == 128)
        return b_kmajor ? launch_pp_one<true, true, E, 192, 128>(p, nblk, st) : launch_pp_one<true, false, E, 192, 128>(p, nblk, st);
    return b_kmajor ? launch_pp_one<true, true, E, 256, 256>(p, nblk, st) : launch_pp_one<true, false, E, 256, 256>(p, nblk, st);
}

}  // namespace xl
