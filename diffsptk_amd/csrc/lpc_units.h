// Internal (non-exported) functions of the LPC kernel families that one translation unit defines and another calls.  Every unit
// that defines or calls one of them includes THIS declaration, so a signature that changes on one side only is a compile error.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dsa {

// ---- csrc/lpc24.hip: tuned Frame -> Window -> LPC forward; dsa_frame_window_lpc_fwd (lpc.hip) checks float32, lpc_order 24,
// 25 <= frame_length <= 512 and that the exact kernel's stretch of 3 P + L samples fits the LDS, else takes its generic route
bool lpc24_fwd_fits(int L, int P);
int lpc24_fwd(const void* x, int64_t B, int64_t T, int64_t N, int L, int P, int left, int pad_mode, const void* w, double eps,
              bool exact_flag, bool scratch_clean, void* scratch, void* out, hipStream_t st);
// ---- csrc/lpc24_bwd.hip: tuned backward of LPC on framed rows for dsa_lpc_bwd (lpc.hip), same conditions
int lpc24_bwd(const void* gout, const void* x, int64_t F, int L, double eps, void* gx, hipStream_t st);

}  // namespace dsa
