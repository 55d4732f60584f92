// Tile geometry of the tuned 512-point STFT kernels: shared by csrc/stft.hip and the packed kernels it includes (stft_pk.h,
// stft_bwd_pk.h, stft_pk_big.h, stft_bwd_pk_big.h).
#pragma once

namespace dsa {

constexpr int kFPW = 4;         // frames per wave (16 lanes each)
constexpr int kTile = kFPW * 257;  // floats in one output tile (4 rows)
// Per-frame stride of the forward kernel's complex tile: ODD, so that the 8-byte transposed reads of the two
// frames a 32-lane LDS service group covers land on opposite bank parities (stride 256: 2-way conflict on
// every one of the 16 reads; PMC: 39 % of the kernel's LDS cycles were conflict cycles).
constexpr int kZS = 272;   // = 16 x 17: the padded transpose tile of a frame (see the forward kernel)

}  // namespace dsa

// The workgroup IS one wave: LDS operations of a wave execute in order, so the phases only need a compiler
// fence.  (__syncthreads() = s_waitcnt vmcnt(0) lgkmcnt(0) + s_barrier: its vmcnt(0) made every pass wait for the
// previous pass's output stores before touching LDS.)
#define DSA_WAVE_SYNC() __builtin_amdgcn_wave_barrier()
