// Shared definitions of the fp16 matrix-pipe kernels (field_h3.hip, field_pw16.hip, bwd16.hip, chain_pw16.hip): the fp16 buffer layouts
// of the half-precision backward, the power-of-two scales, and the weight-unit ring (further down).
//
// "TB16" = tile-blocked fp16 matrix layout of the backward's activation / gradient buffers.  A matrix with one row per sample
// point and CT * 32 channels is stored per 32-point tile and per 32-channel tile as a dense 32 x 32 block of fp16 (2 KiB):
//     element (tile T, channel tile t, point j, channel c)  ->  fp16 index ((T * CT + t) * 32 + j) * 32 + c
// Tiles are the field kernels' own work units (image b, tile k of tiles_per_image = ceil(n_per_image / 32): T = b *
// tiles_per_image + k), so rows past the end of an image exist as rows of their own (G rows there are zero).  Why this
// shape: the producers hold, per lane (point j, half h), 4 consecutive channels of a tile at a time -> one 8-byte store into
// a 2-KiB block that four such instructions complete; the weight-gradient kernel copies a whole tile (all channel tiles of
// 32 points, contiguous) into LDS with linear LDS-DMA and reads MFMA operands out of the 64-byte rows with
// ds_read_b64_tr_b16, conflict-free (bank = 16 j + c / 2 over the 4 rows x 32 channels a half-wave reads).
//
// "COS16": cos(arg) of every slab travels from the storing forward to the chain kernel only, lane for lane (lane (j, h) of the
// wave that owns tile T holds channels 32 t + 8 g + 4 h + e of point j), so it is stored fragment-major -- same size, but every
// wave instruction moves 512 contiguous bytes instead of 16 bytes in each of 32 rows:
//     element (slab m, tile T, channel tile t, quad g, lane, e) -> fp16 index ((((m * tiles + T) * NT + t) * 4 + g) * 64 + lane) * 4 + e
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cnerf {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2_ __attribute__((ext_vector_type(2)));

__device__ __forceinline__ size_t tb16_index(long long tile, int ct, int t, int j, int c) {
    return ((((size_t)tile * ct + t) * 32 + j) * 32) + c;
}

// two fp32 -> packed fp16 pair, round to nearest even (v_cvt_pk_f16_f32 ... the compiler's cast), no saturation needed:
// the callers scale into range
__device__ __forceinline__ uint32_t pk_f16(float a, float b) {
    const f16x2 v = {(_Float16)a, (_Float16)b};
    return __builtin_bit_cast(uint32_t, v);
}

// the two fp16 halves of a packed pair, widened (exact)
__device__ __forceinline__ float half_lo(uint32_t u) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(u & 0xffffu)); }
__device__ __forceinline__ float half_hi(uint32_t u) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(u >> 16)); }

// Weight scale of a packed matrix: S = 2^floor(log2(16384 / max|W|)), so that max|W| S lies in [2^13, 2^14) and both parts of a
// two-part split stay in fp16's normal range.  0 / denormal / huge / NaN -> 1.
__device__ __forceinline__ float pow2_weight_scale(float wmax) {
    if (!(wmax > 1e-30f) || !(wmax < 3e38f)) return 1.0f;
    int e;
    (void)frexpf(16384.0f / wmax, &e);          // 16384 / wmax = m 2^e, m in [0.5, 1)
    return ldexpf(1.0f, e - 1 > 100 ? 100 : e - 1);
}

// Operand scale of a gradient from a bound on it: T = 2^(14 - e) with bound = m 2^e, m in [0.5, 1), so that bound * T lies in
// [2^13, 2^14).  bound == 0 (or denormal / huge) -> 1.
__device__ __forceinline__ float pow2_to_2p14(float bound) {
    const int e = (int)((__float_as_uint(bound) >> 23) & 255u) - 126;
    const int te = 127 + 14 - e;
    return (bound >= 1e-30f && te > 0 && te < 255) ? __uint_as_float((uint32_t)te << 23) : 1.0f;
}

// ---------------------------------------------------------------------------------------------------------------
// The weight-unit ring, common to the eight kernels of the four files above.  One wave owns a 32-point tile; the four waves of a
// block work in lockstep on four tiles of one image and walk one flat sequence of weight units (the A fragments of one or two output
// tiles: a whole number of 1-KiB pieces = 64 lane-linear f16x8 fragments, contiguous in the packed stream).  A unit is
//   copied     into a slot of an LDS ring by LDS-DMA (global_load_lds_dwordx4: 1 KiB per wave instruction, no VGPRs), each wave a
//              quarter of the unit, one unit (two slots) or two units (three slots) ahead of its use, across tile boundaries:
//              dma_unit / dma_unit_ptr;
//   published  at the start of its use by a counted wait and a barrier: LDS-DMA is counted by vmcnt, which retires in issue order,
//              so wait_vmcnt<N>() with N = a lower bound on the vector-memory operations the wave has issued SINCE its share of
//              that copy, then lds_only_barrier() (cnerf_dev.hpp); the same barrier frees the slot that is refilled next.  The wait
//              is written out: the compiler's own fence in front of __syncthreads() once left a barrier without one;
//   read back  lane-linear with ds_read_b128 (conflict-free) as MFMA A fragments through a two-deep register ring, ring[c & 1] =
//              fragment c + 2 once fragment c is taken: tile_kc / input_unit for the PARTS-part fragments of the forward kernels
//              (h3_dev.hpp); the single-part loops of pw_deriv_kernel and the gradient chains are written out where they run,
//              because each schedules different vector work behind its MFMAs (and as one function the chains compile differently).
// Plain LDS stores (constants, the head's fragments) are NOT published by the unit barriers: __syncthreads() once, after them.
// Blocks take groups of four tiles from one eighth of the work per XCD class (group_range(), field_common.hpp); one block per CU is
// launched (launch_per_cu(), cnerf_kernels.hpp).  At its end a block drains its copies (wait_vmcnt<0>, barrier): an LDS-DMA write
// must not land after the block has given its LDS back.
// ---------------------------------------------------------------------------------------------------------------

// One wave instruction moves 1 KiB: lane i's 16 bytes from src_lane land at lds_dst + OFF + 16 i (the instruction offset
// applies to the global and to the LDS address alike).
template <int OFF>
__device__ __forceinline__ void dma_piece(const f16x8* src_lane, f16x8* lds_dst) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src_lane,
                                     (__attribute__((address_space(3))) void*)lds_dst, 16, OFF, 0);
}

// Copy of one weight unit of PIECES pieces: wave w moves the pieces [w PIECES / 4, (w + 1) PIECES / 4).  Two forms that generate
// different code and are therefore kept apart (every kernel keeps the one it was tuned with):
//   dma_unit      instruction-offset form, four pieces per base address (offsets 0, 1, 2, 3 KiB): the forward kernels,
//                 field_h3.hip and field_pw16.hip;
//   dma_unit_ptr  pointer-increment form, one address pair per piece: the gradient chains, bwd16.hip and chain_pw16.hip.
template <int PIECES>
__device__ __forceinline__ void dma_unit(const f16x8* __restrict__ src, f16x8* lds_dst, int wave_u, int lane) {
    static_assert(PIECES % 4 == 0, "four waves share a unit");
    constexpr int PW = PIECES / 4;
    const f16x8* s0 = src + (size_t)wave_u * PW * 64 + lane;
    f16x8* d0 = lds_dst + wave_u * PW * 64;
#pragma unroll
    for (int q = 0; q < (PW + 3) / 4; ++q) {
        const f16x8* sq = s0 + q * 256;
        f16x8* dq = d0 + q * 256;
        if (4 * q + 0 < PW) dma_piece<0>(sq, dq);
        if (4 * q + 1 < PW) dma_piece<1024>(sq, dq);
        if (4 * q + 2 < PW) dma_piece<2048>(sq, dq);
        if (4 * q + 3 < PW) dma_piece<3072>(sq, dq);
    }
}
template <int PIECES>
__device__ __forceinline__ void dma_unit_ptr(const f16x8* __restrict__ src, f16x8* lds_dst, int wave_u, int lane) {
    static_assert(PIECES % 4 == 0, "four waves share a unit");
    constexpr int PW = PIECES / 4;
    const f16x8* s0 = src + (size_t)wave_u * PW * 64 + lane;
    f16x8* d0 = lds_dst + wave_u * PW * 64;
#pragma unroll
    for (int q = 0; q < PW; ++q)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(s0 + q * 64),
                                         (__attribute__((address_space(3))) void*)(d0 + q * 64), 16, 0, 0);
}

}  // namespace cnerf
