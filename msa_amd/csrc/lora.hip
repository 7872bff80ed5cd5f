// Low-rank adapters (LoRA) on the packed Q | K | V projection of an encoder layer (a declared extension; the reference has
// none).  For every targeted third t of qkv [M, 3H]:   qkv_t += s * (x . A_t^T) . B_t^T,   A_t [r, H], B_t [H, r], r in {4, 8, 16}.
//
//   forward   mmbert_lora_qkv_fwd : ONE launch, in place on qkv.  h_t = bf16(x . A_t^T) (fp32 MFMA accumulation), then
//             qkv_t = bf16(fma(s, h_t . B_t^T, float(qkv_t))).
//   backward  mmbert_lora_qkv_bwd : three launches.  (1) g_t = bf16(dqkv_t . B_t), dres_out = bf16(fma(s, sum_t g_t . A_t, float(dres_in)));
//             (2) fp32 partial sums of g_t^T . x and dqkv_t^T . h_t over 128-token slabs; (3) the fold: every output address has ONE adder
//             that takes the slabs in ascending order -- no atomics, the same bits on every device and in either deterministic setting.
//
// A workgroup is 4 waves x 16 token rows.  The rank-r operands are staged ONCE per workgroup into LDS as zero-padded 16-wide tiles (so one
// code path serves r = 4, 8, 16) and all products over H or r run on v_mfma_f32_16x16x32_bf16:
//   * contraction over H (h, g):  D[n][m] = sum_k T[n][k] X[m][k], T = the padded [16, H] tile (LDS), X = 16 rows of x / dqkv_t straight from
//     global memory (16-byte loads).  The result has the token m on the LANE and the rank index n = 4 (lane >> 4) + reg in registers --
//     exactly an operand fragment of the next product, which sums over n: no transpose, no LDS round trip.
//   * contraction over r (the update of qkv_t / dres): the K = 32 instruction with logical k = 4 (lane >> 4) + j for fragment elements j < 4
//     and zeros in j >= 4, on both operands.  Two MFMAs whose operand rows are the columns c0 + 8 (i >> 2) + 4 sub + (i & 3) leave EIGHT
//     consecutive columns of one token row in a lane: the read-modify-write of qkv / dres is a 16-byte load and a 16-byte store.
// The token-axis contraction (dA, dB) has no MFMA form without a transpose of the two big streams (x and dqkv are row-major in the token:
// a fragment would need four tokens of one column in a lane); it runs as fp32 FMAs on 16-byte loads -- r FMAs per loaded element, below
// the memory time of the pass -- a lane owns 8 columns x r rank entries.
//
// The dense seams (the second half of the file) run the same scheme.  SHARED by the two families: the staging helpers and the contraction
// over a staged tile (the tile's row pitch is an argument), lora_expand32, the eight-column update, the input mask, and backward launches 2
// and 3 with their records and launch helper -- the token sums and the fold know streams of a width each, not seams.  SEPARATE: the forward
// and `g` kernels.  The Q | K | V ones stage whole [16, H] tiles of up to three targets (dynamic LDS, row pitch H + 8 elements) and read x
// ONCE for all of them (67.0 us for q + k + v against 3 x 27.7 us as three single-target calls, profiles/lora_dropout_ab.txt); the dense
// ones stage one target in column chunks of a static tile (row pitch LORA_DPITCH) and carry their epilogues.
#include <type_traits>
#include "common.h"
#include "../../include/mmbert_hip.h"

#define LORA_ROWS 64          // token rows per workgroup of the MFMA kernels (4 waves x 16)
#define LORA_SLAB 128         // token rows per partial sum of the weight gradients
#define LORA_LDS_MAX 163840   // 160 KiB per CU (gfx950)

// the input dropout of a seam (the comment block below); rows (dense backward only): local row i is site row rows[i]
struct LoraInDrop { uint32_t stream, thr_pk; float c; int pad; const int32_t* rows; };
struct LoraTarget { const bf16_t* A; const bf16_t* B; int third; int pad; };
struct LoraFwdArgs {
    LoraTarget t[3]; int nt, M, H, r, ldx, ldq, ldh; float s;
    const bf16_t* x; bf16_t* qkv; bf16_t* h;
    LoraInDrop in;
};
struct LoraBwdArgs {
    LoraTarget t[3]; int nt, M, H, r, ldx, lddq, lddi, lddo, recompute; float s;
    const bf16_t* x; const bf16_t* dqkv; const bf16_t* dres_in; bf16_t* dres_out;
    bf16_t* gbuf; bf16_t* hbuf;            // [M, nt * r] each (workspace)
    LoraInDrop in;
};
// One weight-gradient stream of width W (both seam families).  colmajor: out is [W, r] (dB), else [r, W] (dA), whose src is the seam input:
// the only streams the input mask applies to.  part_off: where the stream's [nslab][r W] partial sums start in the workspace (floats)
struct LoraStream { const bf16_t* src; const bf16_t* coef; float* out; size_t part_off; int lds, ldc, colmajor, acc, W, pad; };
// col_lanes: the cap on column lanes (of 8 columns) per workgroup -- it fixes the row-lane count, i.e. the order of the fp32 token sums
struct LoraWArgs { LoraStream st[6]; int ns, M, r, nslab, col_lanes; float s; float* part; LoraInDrop in; };


__device__ __forceinline__ bf16x8 lora_zero8() { bf16x8 z; for (int j = 0; j < 8; ++j) z[j] = (bf16_t)0.0f; return z; }
// the low four fragment elements from 8 bytes, zeros above (logical k = 4 (lane >> 4) + j, see the head of the file)
__device__ __forceinline__ bf16x8 lora_low4(bf16x4 v) {
    bf16x8 o = lora_zero8();
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
    return o;
}
__device__ __forceinline__ bf16x4 lora_round4(f32x4 a) {
    bf16x4 o;
    o[0] = f2bf(a[0]); o[1] = f2bf(a[1]); o[2] = f2bf(a[2]); o[3] = f2bf(a[3]);
    return o;
}

// ---- input dropout of the low-rank branch (the *_drop entry points).  Element (m, k) of a seam input of LOGICAL width K
// (never the row pitch) is kept iff mmb_keep(stream, (uint64) row(m) * K + k, thr16); the base product sees the undropped x.  Every load of
// x is a 16-byte fragment of 8 consecutive columns at a column that is a multiple of 8 and K % 64 == 0, so the fragment is four whole
// element pairs: four hash words, decided on the packed halves.  The roundings:
//   * a dropped element of the fragment becomes +0 -- a SELECT (an AND on the bits), not a product: a NaN in a dropped element stays put;
//   * c = 1 / (1 - thr16 / 65536) is ONE fp32 multiply on the MFMA accumulator of h and of g, before their bf16 rounding: the stored h / g
//     carry c, and dA = s g^T (Kp . x), dB = s dy^T h, dx += s Kp . (g A) need no further factor;
//   * where the mask dropped an element of dx / dres_out, the element keeps the BITS of dx_old / dres_in;
//   * thr16 == 0 runs the DROP = false instantiation of every kernel: the bits of the entry points without dropout (c is not read).
typedef __attribute__((ext_vector_type(4))) uint32_t lora_u32x4;
// the pair index of element (row, 0) of a seam of logical width K (row * K is even); pair indices wrap mod 2^32 as mmb_keep's do
__device__ __forceinline__ uint32_t lora_row_pair(const int32_t* rows, int m, int K) {
    const uint32_t row = rows ? (uint32_t)rows[m] : (uint32_t)m;
    return (uint32_t)(((uint64_t)row * (uint64_t)K) >> 1);
}
// 0xFFFF in the halves of the four words whose elements are DROPPED: the 8 elements from pair index pair0
__device__ __forceinline__ lora_u32x4 lora_drop_bits8(uint32_t stream, uint32_t pair0, uint32_t thr_pk) {
    lora_u32x4 d;
#pragma unroll
    for (int q = 0; q < 4; ++q) d[q] = mmb_drop_mask2(mmb_pair_bits(stream, pair0 + q), thr_pk);
    return d;
}
// the fragment with its dropped elements set to +0
__device__ __forceinline__ bf16x8 lora_drop8(bf16x8 v, uint32_t stream, uint32_t pair0, uint32_t thr_pk) {
    return __builtin_bit_cast(bf16x8, __builtin_bit_cast(lora_u32x4, v) & ~lora_drop_bits8(stream, pair0, thr_pk));
}
// `o` where the mask kept the element, the bits of `old` where it dropped it
__device__ __forceinline__ bf16x8 lora_keep_old8(bf16x8 o, bf16x8 old, uint32_t stream, uint32_t pair0, uint32_t thr_pk) {
    const lora_u32x4 d = lora_drop_bits8(stream, pair0, thr_pk);
    return __builtin_bit_cast(bf16x8, (__builtin_bit_cast(lora_u32x4, o) & ~d) | (__builtin_bit_cast(lora_u32x4, old) & d));
}

// The staging helpers (every thread of the workgroup calls them).  The Q | K | V kernels call them once per target over all of H into that
// target's tile (pitch H + 8); the dense kernels per column chunk into the one static tile (pitch LORA_DPITCH, a constant once inlined).
// T[k][0 .. w) = A[k][c0 .. c0 + w) for k < r, zeros for r <= k < 16 (A: [r, ld] row-major); T's row pitch is `pitch` elements
__device__ __forceinline__ void lora_stage_rows(bf16_t* T, const bf16_t* A, int ld, int c0, int w, int r, int pitch) {
    const int CH = w >> 3, total = 16 * CH;
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
        const int k = idx / CH, c = idx - k * CH;
        bf16x8 v = lora_zero8();
        if (k < r) v = *(const bf16x8*)(A + (size_t)k * ld + c0 + 8 * c);
        *(bf16x8*)(T + (size_t)k * pitch + 8 * c) = v;
    }
}
// T[k][c] = B[c0 + c][k] for k < r, zeros above (B: [N, r] row-major), c < w: the transposed tile for the contraction over N in backward
__device__ __forceinline__ void lora_stage_cols_t(bf16_t* T, const bf16_t* B, int c0, int w, int r, int pitch) {
    for (int c = threadIdx.x; c < w; c += blockDim.x) {
        const bf16_t* src = B + (size_t)(c0 + c) * r;
        bf16_t* dst = T + c;
        for (int k0 = 0; k0 < r; k0 += 4) {
            const bf16x4 v = *(const bf16x4*)(src + k0);
#pragma unroll
            for (int j = 0; j < 4; ++j) dst[(size_t)(k0 + j) * pitch] = v[j];
        }
        for (int k = r; k < 16; ++k) dst[(size_t)k * pitch] = (bf16_t)0.0f;
    }
}
// U[c][k] = B[c0 + c][k] for k < r, zeros for r <= k < 16: 16 elements per column c < w
__device__ __forceinline__ void lora_stage_pad16(bf16_t* U, const bf16_t* B, int c0, int w, int r) {
    for (int c = threadIdx.x; c < w; c += blockDim.x) {
        const bf16_t* src = B + (size_t)(c0 + c) * r;
        bf16x8 lo = lora_zero8(), hi = lora_zero8();
        if (r == 16) { lo = *(const bf16x8*)src; hi = *(const bf16x8*)(src + 8); }
        else if (r == 8) lo = *(const bf16x8*)src;
        else lo = lora_low4(*(const bf16x4*)src);
        bf16_t* dst = U + (size_t)c * 16;
        *(bf16x8*)dst = lo; *(bf16x8*)(dst + 8) = hi;
    }
}
// U[c][k] = A[k][c0 + c] for k < r, zeros above (A: [r, ld] row-major), c < w: the transposed form, for the input gradient
__device__ __forceinline__ void lora_stage_pad16_t(bf16_t* U, const bf16_t* A, int ld, int c0, int w, int r) {
    const int CH = w >> 3, total = 16 * CH;
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
        const int k = idx / CH, c = idx - k * CH;
        bf16x8 v = lora_zero8();
        if (k < r) v = *(const bf16x8*)(A + (size_t)k * ld + c0 + 8 * c);
        bf16_t* dst = U + (size_t)(8 * c) * 16 + k;
#pragma unroll
        for (int j = 0; j < 8; ++j) dst[j * 16] = v[j];
    }
}

// acc[n][m] += sum_k T[n][k] X[m][k] over k < w, in 32-wide blocks in ascending k: T = a staged tile of row pitch `pitch`, X = the wave's 16
// rows (xrow: this lane's row, at the tile's first column).  DROP: X is read under the input mask; p0 = the pair index of this lane's first
// fragment (row pair + (first column + 8 g) / 2)
template <bool DROP>
__device__ __forceinline__ void lora_contract_chunk(f32x4& acc, const bf16_t* T, const bf16_t* xrow, int w, int pitch, int lane, const LoraInDrop& d, uint32_t p0) {
    const int i = lane & 15, g = lane >> 4;
    const bf16_t* tr = T + (size_t)i * pitch + 8 * g;
    const bf16_t* xr = xrow + 8 * g;
    for (int k = 0; k < w; k += 32) {
        bf16x8 xf = *(const bf16x8*)(xr + k);
        if constexpr (DROP) xf = lora_drop8(xf, d.stream, p0 + (uint32_t)(k >> 1), d.thr_pk);
        const bf16x8 tf = *(const bf16x8*)(tr + k);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tf, xf, acc, 0, 0, 0);
    }
}
// the same for the nt targets at once under the input mask: the targets read the same x and share its mask (one mask per seam INPUT), so
// the masked fragment is formed ONCE per K step; each accumulator takes the k blocks in lora_contract_chunk's order, then c (rowpair:
// lora_row_pair of this lane's row; the tiles at pitch H + 8)
__device__ __forceinline__ void lora_contract_h_drop(const bf16_t* T, const bf16_t* xrow, int H, int nt, int lane, const LoraInDrop& d, uint32_t rowpair, f32x4 acc[3]) {
    const int i = lane & 15, g = lane >> 4;
    const bf16_t* tr = T + (size_t)i * (H + 8) + 8 * g;
    const bf16_t* xr = xrow + 8 * g;
    const uint32_t p0 = rowpair + 4 * g;
#pragma unroll
    for (int ti = 0; ti < 3; ++ti) acc[ti] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < H; k0 += 32) {
        const bf16x8 xf = lora_drop8(*(const bf16x8*)(xr + k0), d.stream, p0 + (uint32_t)(k0 >> 1), d.thr_pk);
#pragma unroll
        for (int ti = 0; ti < 3; ++ti)
            if (ti < nt) acc[ti] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(tr + (size_t)ti * 16 * (H + 8) + k0), xf, acc[ti], 0, 0, 0);
    }
#pragma unroll
    for (int ti = 0; ti < 3; ++ti) acc[ti] *= d.c;
}

// the two MFMAs of one 32-column block: d[sub][reg] = sum_k U[c0 + 8 g + 4 sub + reg][k] v[m][k]  (token m = lane & 15, g = lane >> 4)
__device__ __forceinline__ void lora_expand32(const bf16_t* U, int c0, bf16x8 vf, int lane, f32x4& d0, f32x4& d1) {
    const int i = lane & 15, g = lane >> 4;
    const bf16_t* u = U + (size_t)(c0 + 8 * (i >> 2) + (i & 3)) * 16 + 4 * g;
    const bf16x8 u0 = lora_low4(*(const bf16x4*)u), u1 = lora_low4(*(const bf16x4*)(u + 4 * 16));
    d0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(u0, vf, d0, 0, 0, 0);
    d1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(u1, vf, d1, 0, 0, 0);
}
// the update of the eight columns lora_expand32 left in this lane: o[j] = bf16(fma(s, d[j], float(old[j])))
__device__ __forceinline__ bf16x8 lora_update8(float s, f32x4 d0, f32x4 d1, bf16x8 old) {
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) { o[j] = f2bf(fmaf(s, d0[j], bf2f(old[j]))); o[4 + j] = f2bf(fmaf(s, d1[j], bf2f(old[4 + j]))); }
    return o;
}

template <bool DROP>
__global__ __launch_bounds__(256) void lora_qkv_fwd_kernel(const LoraFwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* T = (bf16_t*)smem;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
    const int H = a.H, HP = H + 8, r = a.r, nt = a.nt;
    const int m = blockIdx.x * LORA_ROWS + wave * 16 + (lane & 15);
    const bool live = m < a.M;
    const bool wave_live = blockIdx.x * LORA_ROWS + wave * 16 < a.M;
    const int mr = live ? m : a.M - 1;                              // rows past M read row M - 1 and store nothing
    for (int ti = 0; ti < nt; ++ti) lora_stage_rows(T + (size_t)ti * 16 * HP, a.t[ti].A, H, 0, H, r, HP);
    __syncthreads();
    bf16x8 hf[3];
    for (int ti = 0; ti < 3; ++ti) hf[ti] = lora_zero8();
    if (wave_live) {
        const bf16_t* xrow = a.x + (size_t)mr * a.ldx;
        f32x4 hacc[3];
        if constexpr (DROP) lora_contract_h_drop(T, xrow, H, nt, lane, a.in, lora_row_pair(nullptr, mr, H), hacc);
#pragma unroll
        for (int ti = 0; ti < 3; ++ti) {
            if (ti < nt) {
                if constexpr (!DROP) {
                    hacc[ti] = (f32x4){0.f, 0.f, 0.f, 0.f};
                    lora_contract_chunk<false>(hacc[ti], T + (size_t)ti * 16 * HP, xrow, H, HP, lane, a.in, 0u);
                }
                const bf16x4 hb = lora_round4(hacc[ti]);
                hf[ti] = lora_low4(hb);
                if (a.h && live && 4 * g < r) *(bf16x4*)(a.h + (size_t)m * a.ldh + ti * r + 4 * g) = hb;
            }
        }
    }
    __syncthreads();
    for (int ti = 0; ti < nt; ++ti) lora_stage_pad16(T + (size_t)ti * H * 16, a.t[ti].B, 0, H, r);
    __syncthreads();
    if (!wave_live) return;
#pragma unroll
    for (int ti = 0; ti < 3; ++ti) {
        if (ti >= nt) break;
        const bf16_t* U = T + (size_t)ti * H * 16;
        bf16_t* q = a.qkv + (size_t)mr * a.ldq + (size_t)a.t[ti].third * H + 8 * g;

        for (int c0 = 0; c0 < H; c0 += 32) {
            const bf16x8 old = *(const bf16x8*)(q + c0);
            f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = {0.f, 0.f, 0.f, 0.f};
            lora_expand32(U, c0, hf[ti], lane, d0, d1);
            const bf16x8 o = lora_update8(a.s, d0, d1, old);
            if (live) *(bf16x8*)(q + c0) = o;
        }
    }
}

// backward launch 1: g (and h, when it is recomputed) into the workspace, and the input-gradient part
template <bool DROP>
__global__ __launch_bounds__(256) void lora_qkv_bwd_g_kernel(const LoraBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* T = (bf16_t*)smem;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
    const int H = a.H, HP = H + 8, r = a.r, nt = a.nt;
    const int m = blockIdx.x * LORA_ROWS + wave * 16 + (lane & 15);
    const bool live = m < a.M;
    const bool wave_live = blockIdx.x * LORA_ROWS + wave * 16 < a.M;
    const int mr = live ? m : a.M - 1;
    const int ldw = nt * r;
    if (a.recompute) {                                               // h = bf16(x . A^T), as forward formed it
        for (int ti = 0; ti < nt; ++ti) lora_stage_rows(T + (size_t)ti * 16 * HP, a.t[ti].A, H, 0, H, r, HP);
        __syncthreads();
        if (wave_live) {
            const bf16_t* xrow = a.x + (size_t)mr * a.ldx;
            f32x4 hacc[3];
            if constexpr (DROP) lora_contract_h_drop(T, xrow, H, nt, lane, a.in, lora_row_pair(nullptr, mr, H), hacc);
#pragma unroll
            for (int ti = 0; ti < 3; ++ti) {
                if (ti < nt) {
                    if constexpr (!DROP) {
                        hacc[ti] = (f32x4){0.f, 0.f, 0.f, 0.f};
                        lora_contract_chunk<false>(hacc[ti], T + (size_t)ti * 16 * HP, xrow, H, HP, lane, a.in, 0u);
                    }
                    const bf16x4 hb = lora_round4(hacc[ti]);
                    if (live && 4 * g < r) *(bf16x4*)(a.hbuf + (size_t)m * ldw + ti * r + 4 * g) = hb;
                }
            }
        }
        __syncthreads();
    }
    for (int ti = 0; ti < nt; ++ti) lora_stage_cols_t(T + (size_t)ti * 16 * HP, a.t[ti].B, 0, H, r, HP);
    __syncthreads();
    bf16x8 gf[3];
    for (int ti = 0; ti < 3; ++ti) gf[ti] = lora_zero8();
    if (wave_live) {
#pragma unroll
        for (int ti = 0; ti < 3; ++ti) {
            if (ti < nt) {
                const bf16_t* drow = a.dqkv + (size_t)mr * a.lddq + (size_t)a.t[ti].third * H;
                f32x4 gacc = {0.f, 0.f, 0.f, 0.f};
                lora_contract_chunk<false>(gacc, T + (size_t)ti * 16 * HP, drow, H, HP, lane, a.in, 0u);
                if constexpr (DROP) gacc *= a.in.c;                  // g carries c: dA and the input gradient need no further factor
                const bf16x4 gb = lora_round4(gacc);
                gf[ti] = lora_low4(gb);
                if (live && 4 * g < r) *(bf16x4*)(a.gbuf + (size_t)m * ldw + ti * r + 4 * g) = gb;
            }
        }
    }
    if (!a.dres_out) return;                                         // (uniform over the grid)
    __syncthreads();
    for (int ti = 0; ti < nt; ++ti) lora_stage_pad16_t(T + (size_t)ti * H * 16, a.t[ti].A, H, 0, H, r);
    __syncthreads();
    if (!wave_live) return;
    const bf16_t* din = a.dres_in + (size_t)mr * a.lddi + 8 * g;
    bf16_t* dout = a.dres_out + (size_t)mr * a.lddo + 8 * g;
    const uint32_t p0 = DROP ? lora_row_pair(nullptr, mr, H) + 4 * g : 0u;

    for (int c0 = 0; c0 < H; c0 += 32) {
        const bf16x8 old = *(const bf16x8*)(din + c0);
        f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ti = 0; ti < 3; ++ti)
            if (ti < nt) lora_expand32(T + (size_t)ti * H * 16, c0, gf[ti], lane, d0, d1);
        bf16x8 o = lora_update8(a.s, d0, d1, old);
        if constexpr (DROP) o = lora_keep_old8(o, old, a.in.stream, p0 + (uint32_t)(c0 >> 1), a.in.thr_pk);
        if (live) *(bf16x8*)(dout + c0) = o;
    }
}

// backward launch 2, both seam families: part[stream][slab][k, c] = sum over the slab's tokens m of coef[m][k] * src[m][c]  (fp32; not yet
// scaled by s).  A lane owns 8 columns and all R rank entries; the column axis runs over blockIdx.z in blocks of CHW = min(W / 8, col_lanes)
// column lanes, and the workgroup's 256 / CHW row lanes take interleaved tokens and are added in row-lane order.  col_lanes is the caller's:
// 256 from the Q | K | V entry points (one workgroup per slab and stream up to H = 2048), 128 from the dense ones (an I-wide stream runs on 3
// (bert-base) or 4 (bert-large) workgroups per slab with two row lanes each).
// DROP: the dA streams (src = x, the seam input) read x under the input mask of the SITE rows (in.rows[m] on gathered operands, m itself when
// it is null); the dB streams read dy / dqkv and h as they are.
template <int R, bool DROP>
__global__ __launch_bounds__(256) void lora_bwd_w_kernel(const LoraWArgs a) {
    __shared__ __attribute__((aligned(16))) float red[256 * 8];
    const LoraStream& st = a.st[blockIdx.y];
    const int W = st.W, CH = W >> 3;
    const bool masked = DROP && !st.colmajor;                        // (uniform over the workgroup)
    const int CHW = min(CH, a.col_lanes), RL = 256 / CHW;
    const int cb = blockIdx.z * CHW;
    if (cb >= CH) return;                                            // (uniform over the workgroup: the narrower stream has fewer column blocks)
    const int cc = threadIdx.x % CHW, rl = threadIdx.x / CHW;
    const int mbeg = blockIdx.x * LORA_SLAB, mend = min(a.M, mbeg + LORA_SLAB);
    float* part = a.part + st.part_off + (size_t)blockIdx.x * (size_t)(R * W);
    const int c = cb + cc;
    const bool act = rl < RL && c < CH;
    float acc[R][8];
#pragma unroll
    for (int k = 0; k < R; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[k][j] = 0.f;
    // The token sums of this lane.  gather: the mask of row m is that of site row in.rows[m]; else that of row m.  Two loops, chosen outside
    // them: with the row list's null test inside the loop the four loads of a round no longer go out together, which cost the Q | K | V
    // seam (never a row list) 2 us of 77 at 18 400 rows (profiles/lora_kernels_ab.txt)
    auto sums = [&](auto gather) {
        const int32_t* rows = decltype(gather)::value ? a.in.rows : nullptr;
        const bf16_t* src = st.src + 8 * c;
        int m = mbeg + rl;
        for (; m + 3 * RL < mend; m += 4 * RL) {                      // four independent 16-byte loads in flight
            bf16x8 v[4];
            bf16x4 w[4][R / 4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                v[u] = *(const bf16x8*)(src + (size_t)(m + u * RL) * st.lds);
                if constexpr (DROP)
                    if (masked) v[u] = lora_drop8(v[u], a.in.stream, lora_row_pair(rows, m + u * RL, W) + 4 * c, a.in.thr_pk);
#pragma unroll
                for (int q = 0; q < R / 4; ++q) w[u][q] = *(const bf16x4*)(st.coef + (size_t)(m + u * RL) * st.ldc + 4 * q);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int k = 0; k < R; ++k) {
                    const float wk = bf2f(w[u][k >> 2][k & 3]);
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[k][j] = fmaf(wk, bf2f(v[u][j]), acc[k][j]);
                }
        }
        for (; m < mend; m += RL) {
            bf16x8 v = *(const bf16x8*)(src + (size_t)m * st.lds);
            if constexpr (DROP)
                if (masked) v = lora_drop8(v, a.in.stream, lora_row_pair(rows, m, W) + 4 * c, a.in.thr_pk);
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const float wk = bf2f(st.coef[(size_t)m * st.ldc + k]);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[k][j] = fmaf(wk, bf2f(v[j]), acc[k][j]);
            }
        }
    };
    if (act) {
        if (DROP && masked && a.in.rows) sums(std::true_type{});
        else sums(std::false_type{});
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {                                    // row lanes 1 .. RL-1 are added onto row lane 0, in order
        if (act && rl > 0) {
            *(float4*)(red + (size_t)threadIdx.x * 8) = make_float4(acc[k][0], acc[k][1], acc[k][2], acc[k][3]);
            *(float4*)(red + (size_t)threadIdx.x * 8 + 4) = make_float4(acc[k][4], acc[k][5], acc[k][6], acc[k][7]);
        }
        __syncthreads();
        if (act && rl == 0) {
            for (int q = 1; q < RL; ++q)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[k][j] += red[(size_t)(q * CHW + cc) * 8 + j];
        }
        __syncthreads();
    }
    if (act && rl == 0) {
        if (st.colmajor) {                                           // [W, R]: R consecutive floats per column
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int k = 0; k < R; k += 4)
                    *(float4*)(part + (size_t)(8 * c + j) * R + k) = make_float4(acc[k][j], acc[k + 1][j], acc[k + 2][j], acc[k + 3][j]);
        } else {                                                     // [R, W]
#pragma unroll
            for (int k = 0; k < R; ++k) {
                *(float4*)(part + (size_t)k * W + 8 * c) = make_float4(acc[k][0], acc[k][1], acc[k][2], acc[k][3]);
                *(float4*)(part + (size_t)k * W + 8 * c + 4) = make_float4(acc[k][4], acc[k][5], acc[k][6], acc[k][7]);
            }
        }
    }
}

// backward launch 3: out[e] = (acc ? out[e] : 0) + s * (slab 0 + slab 1 + ... in ascending order); a lane owns 4 consecutive elements
__global__ __launch_bounds__(256) void lora_fold_kernel(const LoraWArgs a) {
    const LoraStream& st = a.st[blockIdx.y];
    const size_t n = (size_t)a.r * st.W;
    const size_t e = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (e >= n) return;
    const float* p = a.part + st.part_off + e;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    int q = 0;
    for (; q + 4 <= a.nslab; q += 4) {                               // loads four slabs ahead, adds in order
        float4 t[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) t[u] = *(const float4*)(p + (size_t)(q + u) * n);
#pragma unroll
        for (int u = 0; u < 4; ++u) { s.x += t[u].x; s.y += t[u].y; s.z += t[u].z; s.w += t[u].w; }
    }
    for (; q < a.nslab; ++q) {
        const float4 t = *(const float4*)(p + (size_t)q * n);
        s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
    }
    float4* o = (float4*)(st.out + e);
    float4 v = make_float4(a.s * s.x, a.s * s.y, a.s * s.z, a.s * s.w);
    if (st.acc) { const float4 w = *o; v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w; }
    *o = v;
}

static inline bool lora_shape_ok(int M, int H, int r, int targets) {
    return M >= 0 && H > 0 && (H & 63) == 0 && (r == 4 || r == 8 || r == 16) && targets >= 1 && targets <= 7;
}
static inline int lora_count(int targets) { return (targets & 1) + ((targets >> 1) & 1) + ((targets >> 2) & 1); }
static inline size_t lora_lds_bytes(int nt, int H) { return (size_t)nt * 16 * (size_t)(H + 8) * sizeof(bf16_t); }
static inline size_t lora_up16(size_t b) { return (b + 15) & ~(size_t)15; }
static inline bool lora_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline bool lora_al8(const void* p) { return ((uintptr_t)p & 7) == 0; }

static int lora_targets(LoraTarget* t, int targets, const void* const* A, const void* const* B) {
    int nt = 0;
    for (int k = 0; k < 3; ++k) {
        if (!((targets >> k) & 1)) continue;
        if (!A || !B || !A[k] || !B[k] || !lora_al16(A[k]) || !lora_al16(B[k])) return -1;
        t[nt].A = (const bf16_t*)A[k]; t[nt].B = (const bf16_t*)B[k]; t[nt].third = k; t[nt].pad = 0;
        ++nt;
    }
    return nt;
}

// the input-dropout triple of the *_drop entry points: thr16 <= 65535, scale finite and > 0 (thr16 == 0: the triple is otherwise unused)
static inline bool lora_in_drop_ok(unsigned thr16, float scale) { return thr16 <= 65535u && scale > 0.0f && scale < INFINITY; }
static inline LoraInDrop lora_in_drop(unsigned in_stream, unsigned thr16, float scale, const int32_t* rows) {
    LoraInDrop d = {};
    d.stream = in_stream; d.thr_pk = mmb_thr_packed(thr16); d.c = scale; d.rows = rows;
    return d;
}

// launch 1 of either direction: one workgroup per LORA_ROWS token rows; more than 64 KiB of dynamic LDS needs the kernel's one-time opt-in
template <auto KERNEL, typename Args>
static int lora_rows_launch(hipStream_t stream, const Args& a, size_t lds) {
    if (lds > 65536) {
        static std::atomic<unsigned long long> done{0};
        const int e = mmb_allow_lds((const void*)KERNEL, (int)lds, done);
        if (e) return e;
    }
    hipLaunchKernelGGL(KERNEL, dim3((a.M + LORA_ROWS - 1) / LORA_ROWS), dim3(256), lds, stream, a);
    MMB_CHECK_LAUNCH();
    return 0;
}
// backward launches 2 and 3 over the streams of w; wmax = the widest of them
template <bool DROP>
static int lora_bwd_w_launch(hipStream_t stream, const LoraWArgs& w, int wmax) {
    const dim3 grid(w.nslab, w.ns, (wmax / 8 + w.col_lanes - 1) / w.col_lanes);
    if (w.r == 4) hipLaunchKernelGGL((lora_bwd_w_kernel<4, DROP>), grid, dim3(256), 0, stream, w);
    else if (w.r == 8) hipLaunchKernelGGL((lora_bwd_w_kernel<8, DROP>), grid, dim3(256), 0, stream, w);
    else hipLaunchKernelGGL((lora_bwd_w_kernel<16, DROP>), grid, dim3(256), 0, stream, w);
    MMB_CHECK_LAUNCH();
    hipLaunchKernelGGL(lora_fold_kernel, dim3((unsigned)(((size_t)w.r * wmax / 4 + 255) / 256), w.ns), dim3(256), 0, stream, w);
    MMB_CHECK_LAUNCH();
    return 0;
}

static int lora_qkv_fwd_impl(hipStream_t stream, const void* x, int ldx, void* qkv, int ldq, int M, int H, int r, int targets,
                             const void* const* A, const void* const* B, float scale, void* h_out, int ldh,
                             unsigned in_stream, unsigned in_thr16, float in_scale) {
    if (!lora_shape_ok(M, H, r, targets) || !lora_in_drop_ok(in_thr16, in_scale)) return -1;
    if (M == 0) return 0;
    LoraFwdArgs a = {};
    a.nt = lora_targets(a.t, targets, A, B);
    if (a.nt < 0) return -1;
    if (!x || !qkv || !lora_al16(x) || !lora_al16(qkv) || ldx < H || (ldx & 7) || ldq < 3 * H || (ldq & 7)) return -1;
    if (h_out && (!lora_al8(h_out) || ldh < a.nt * r || (ldh & 3))) return -1;
    const size_t lds = lora_lds_bytes(a.nt, H);
    if (lds > LORA_LDS_MAX) return -2;
    a.M = M; a.H = H; a.r = r; a.ldx = ldx; a.ldq = ldq; a.ldh = ldh; a.s = scale;
    a.x = (const bf16_t*)x; a.qkv = (bf16_t*)qkv; a.h = (bf16_t*)h_out;
    a.in = lora_in_drop(in_stream, in_thr16, in_scale, nullptr);
    return in_thr16 ? lora_rows_launch<lora_qkv_fwd_kernel<true>>(stream, a, lds) : lora_rows_launch<lora_qkv_fwd_kernel<false>>(stream, a, lds);
}

extern "C" {

int mmbert_lora_qkv_fwd(hipStream_t stream, const void* x, int ldx, void* qkv, int ldq, int M, int H, int r, int targets,
                        const void* const* A, const void* const* B, float scale, void* h_out, int ldh) {
    return lora_qkv_fwd_impl(stream, x, ldx, qkv, ldq, M, H, r, targets, A, B, scale, h_out, ldh, 0u, 0u, 1.0f);
}

int mmbert_lora_qkv_fwd_drop(hipStream_t stream, const void* x, int ldx, void* qkv, int ldq, int M, int H, int r, int targets,
                             const void* const* A, const void* const* B, float scale, void* h_out, int ldh,
                             unsigned in_stream, unsigned in_thr16, float in_scale) {
    return lora_qkv_fwd_impl(stream, x, ldx, qkv, ldq, M, H, r, targets, A, B, scale, h_out, ldh, in_stream, in_thr16, in_scale);
}

// [partial sums: 2 nt streams x slabs x r H floats][g: M x nt r bf16][h, when backward recomputes it: the same]; 0 for M == 0 or a bad shape
size_t mmbert_lora_qkv_bwd_workspace(int M, int H, int r, int targets) {
    if (!lora_shape_ok(M, H, r, targets) || M == 0) return 0;
    const int nt = lora_count(targets);
    const size_t nslab = (size_t)(M + LORA_SLAB - 1) / LORA_SLAB;
    const size_t part = (size_t)2 * nt * nslab * (size_t)r * H * sizeof(float);
    const size_t gb = lora_up16((size_t)M * nt * r * sizeof(bf16_t));
    return part + 2 * gb;
}

static int lora_qkv_bwd_impl(hipStream_t stream, const void* dqkv, int lddq, const void* x, int ldx, const void* h, int ldh, int M, int H, int r,
                             int targets, const void* const* A, const void* const* B, float scale, const void* dres_in, int lddi,
                             void* dres_out, int lddo, float* const* gA, float* const* gB, int accumulate, void* workspace,
                             unsigned in_stream, unsigned in_thr16, float in_scale) {
    if (!lora_shape_ok(M, H, r, targets) || !lora_in_drop_ok(in_thr16, in_scale)) return -1;
    if (M == 0) return 0;
    LoraBwdArgs a = {};
    a.nt = lora_targets(a.t, targets, A, B);
    if (a.nt < 0) return -1;
    const int nt = a.nt;
    if (!dqkv || !x || !lora_al16(dqkv) || !lora_al16(x) || lddq < 3 * H || (lddq & 7) || ldx < H || (ldx & 7)) return -1;
    if (h && (!lora_al8(h) || ldh < nt * r || (ldh & 3))) return -1;
    if (dres_out && (!dres_in || dres_in == dres_out || !lora_al16(dres_in) || !lora_al16(dres_out) || lddi < H || (lddi & 7) || lddo < H || (lddo & 7))) return -1;
    if (!workspace || !lora_al16(workspace)) return -3;
    const size_t lds = lora_lds_bytes(nt, H);
    if (lds > LORA_LDS_MAX) return -2;
    const int nslab = (M + LORA_SLAB - 1) / LORA_SLAB;
    const size_t part = (size_t)2 * nt * nslab * (size_t)r * H * sizeof(float);
    const size_t gb = lora_up16((size_t)M * nt * r * sizeof(bf16_t));
    a.M = M; a.H = H; a.r = r; a.ldx = ldx; a.lddq = lddq; a.lddi = lddi; a.lddo = lddo; a.s = scale;
    a.x = (const bf16_t*)x; a.dqkv = (const bf16_t*)dqkv; a.dres_in = (const bf16_t*)dres_in; a.dres_out = (bf16_t*)dres_out;
    a.gbuf = (bf16_t*)((char*)workspace + part); a.hbuf = (bf16_t*)((char*)workspace + part + gb);
    // the weight-gradient streams that run: a target's dA needs g and x, its dB needs dqkv and h
    LoraWArgs w = {};
    bool need_h = false;
    for (int ti = 0; ti < nt; ++ti) {
        const int k = a.t[ti].third;
        float* ga = gA ? gA[k] : nullptr;
        float* gb_ = gB ? gB[k] : nullptr;
        if (ga) {
            if (!lora_al16(ga)) return -1;
            LoraStream& s = w.st[w.ns++];
            s.src = a.x; s.lds = ldx; s.coef = a.gbuf + ti * r; s.ldc = nt * r; s.out = ga; s.colmajor = 0;
        }
        if (gb_) {
            if (!lora_al16(gb_)) return -1;
            LoraStream& s = w.st[w.ns++];
            s.src = a.dqkv + (size_t)k * H; s.lds = lddq; s.out = gb_; s.colmajor = 1;
            if (h) { s.coef = (const bf16_t*)h + ti * r; s.ldc = ldh; }
            else { s.coef = a.hbuf + ti * r; s.ldc = nt * r; need_h = true; }
        }
    }
    a.recompute = need_h ? 1 : 0;
    if (!dres_out && w.ns == 0) return 0;                            // nothing asked for
    a.in = w.in = lora_in_drop(in_stream, in_thr16, in_scale, nullptr);
    const int e = in_thr16 ? lora_rows_launch<lora_qkv_bwd_g_kernel<true>>(stream, a, lds) : lora_rows_launch<lora_qkv_bwd_g_kernel<false>>(stream, a, lds);
    if (e || w.ns == 0) return e;
    for (int i = 0; i < w.ns; ++i) {                                 // every stream is H wide: stream i's partial sums follow stream i - 1's
        w.st[i].W = H; w.st[i].part_off = (size_t)i * nslab * (size_t)r * H; w.st[i].acc = accumulate ? 1 : 0;
    }
    w.M = M; w.r = r; w.nslab = nslab; w.col_lanes = 256; w.s = scale; w.part = (float*)workspace;
    return in_thr16 ? lora_bwd_w_launch<true>(stream, w, H) : lora_bwd_w_launch<false>(stream, w, H);
}

int mmbert_lora_qkv_bwd(hipStream_t stream, const void* dqkv, int lddq, const void* x, int ldx, const void* h, int ldh, int M, int H, int r,
                        int targets, const void* const* A, const void* const* B, float scale, const void* dres_in, int lddi,
                        void* dres_out, int lddo, float* const* gA, float* const* gB, int accumulate, void* workspace) {
    return lora_qkv_bwd_impl(stream, dqkv, lddq, x, ldx, h, ldh, M, H, r, targets, A, B, scale, dres_in, lddi, dres_out, lddo, gA, gB, accumulate,
                             workspace, 0u, 0u, 1.0f);
}

int mmbert_lora_qkv_bwd_drop(hipStream_t stream, const void* dqkv, int lddq, const void* x, int ldx, const void* h, int ldh, int M, int H, int r,
                             int targets, const void* const* A, const void* const* B, float scale, const void* dres_in, int lddi,
                             void* dres_out, int lddo, float* const* gA, float* const* gB, int accumulate, void* workspace,
                             unsigned in_stream, unsigned in_thr16, float in_scale) {
    return lora_qkv_bwd_impl(stream, dqkv, lddq, x, ldx, h, ldh, M, H, r, targets, A, B, scale, dres_in, lddi, dres_out, lddo, gA, gB, accumulate,
                             workspace, in_stream, in_thr16, in_scale);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------------------
// Adapters on the three remaining dense seams of an encoder layer (attention.output.dense, intermediate.dense, output.dense; DESIGN.md
// S3.15): y [M, N] behind the projection's own GEMM, x [M, K] its input, A [r, K], B [N, r], K != N in general.  The fragment scheme, the
// helpers and backward launches 2 and 3 are the ones above (one stream of width K for dA, one of width N for dB, col_lanes = 128); these
// forward and `g` kernels differ from the Q | K | V ones in:
//   * A and B are staged in column CHUNKS of LORA_DCHUNK (768) columns into ONE static 24.8 KB tile, so the LDS footprint does not grow
//     with the FFN width and several workgroups share a CU.  The fp32 accumulator of a contraction lives across the chunks: k ascends in
//     32-wide blocks exactly as over one whole tile, chunking changes no rounding.
//   * the epilogue of the forward update: ADD  y = bf16(fma(s * c, p, float(y))), c = drop_scale on the elements the GEMM's dropout kept
//     (same stream, threshold, flat index m * N + n) and the element untouched where it dropped;  GELU  w = fma(s, p, float(y)),
//     aux = bf16(w), y = bf16(gelu(w)).
//   * the input gradient is updated IN PLACE, optionally times gelu'(float(u)).
#define LORA_DCHUNK 768
#define LORA_DPITCH (LORA_DCHUNK + 8)
#define LORA_DTILE (16 * LORA_DPITCH)                      // elements; >= LORA_DCHUNK * 16 (the [columns, 16] form)

struct LoraDenseFwdArgs {
    const bf16_t* x; bf16_t* y; const bf16_t* A; const bf16_t* B; bf16_t* aux; bf16_t* h;
    int M, K, N, r, ldx, ldy, ldaux, ldh, gelu;
    float s, sc;                                           // sc = s * drop_scale (ONE fp32 product, formed on the host)
    uint32_t dstream, thr16, thr_pk;
    LoraInDrop in;                                         // the dropout of the adapter's INPUT x (the triple above: the GEMM's, on y)
};
struct LoraDenseBwdArgs {
    const bf16_t* dy; const bf16_t* x; const bf16_t* A; const bf16_t* B; const bf16_t* u; bf16_t* dx; bf16_t* gbuf; bf16_t* hbuf;
    int M, K, N, r, lddy, ldx, lddx, ldu, recompute; float s;
    LoraInDrop in;
};

// h = x . A^T of the wave's 16 rows over all of K, chunk by chunk (every thread of the workgroup calls it: it synchronises).  DROP: x under
// the input mask (rowpair: lora_row_pair of this lane's row) and c on the finished accumulator
template <bool DROP>
__device__ __forceinline__ f32x4 lora_dense_contract(bf16_t* T, const bf16_t* W, bool rows_form, const bf16_t* xrow, int K, int r, bool wave_live, int lane,
                                                     const LoraInDrop& d, uint32_t rowpair) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += LORA_DCHUNK) {
        const int w = min(LORA_DCHUNK, K - k0);
        if (rows_form) lora_stage_rows(T, W, K, k0, w, r, LORA_DPITCH);
        else lora_stage_cols_t(T, W, k0, w, r, LORA_DPITCH);
        __syncthreads();
        if (wave_live) lora_contract_chunk<DROP>(acc, T, xrow + k0, w, LORA_DPITCH, lane, d, rowpair + (uint32_t)((k0 + 8 * (lane >> 4)) >> 1));
        __syncthreads();
    }
    if constexpr (DROP) acc *= d.c;
    return acc;
}

template <bool DROP>
__global__ __launch_bounds__(256) void lora_dense_fwd_kernel(const LoraDenseFwdArgs a) {
    __shared__ __attribute__((aligned(16))) bf16_t T[LORA_DTILE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
    const int K = a.K, N = a.N, r = a.r;
    const int m = blockIdx.x * LORA_ROWS + wave * 16 + (lane & 15);
    const bool live = m < a.M;
    const bool wave_live = blockIdx.x * LORA_ROWS + wave * 16 < a.M;
    const int mr = live ? m : a.M - 1;                              // rows past M read row M - 1 and store nothing
    const bf16x4 hb = lora_round4(lora_dense_contract<DROP>(T, a.A, true, a.x + (size_t)mr * a.ldx, K, r, wave_live, lane, a.in,
                                                            DROP ? lora_row_pair(nullptr, mr, K) : 0u));
    const bf16x8 hf = lora_low4(hb);
    if (a.h && live && 4 * g < r) *(bf16x4*)(a.h + (size_t)m * a.ldh + 4 * g) = hb;
    bf16_t* yrow = a.y + (size_t)mr * a.ldy + 8 * g;
    bf16_t* arow = a.aux ? a.aux + (size_t)mr * a.ldaux + 8 * g : nullptr;
    const uint64_t flat = (uint64_t)mr * (uint64_t)N + (uint64_t)(8 * g);   // the GEMM's dropout index: LOGICAL column count, not the pitch
    for (int n0 = 0; n0 < N; n0 += LORA_DCHUNK) {
        const int w = min(LORA_DCHUNK, N - n0);
        lora_stage_pad16(T, a.B, n0, w, r);
        __syncthreads();
        if (wave_live) {
            for (int c0 = 0; c0 < w; c0 += 32) {
                const bf16x8 old = *(const bf16x8*)(yrow + n0 + c0);
                f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = {0.f, 0.f, 0.f, 0.f};
                lora_expand32(T, c0, hf, lane, d0, d1);
                float p[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) { p[j] = d0[j]; p[4 + j] = d1[j]; }
                bf16x8 o;
                if (a.gelu) {
                    bf16x8 uo;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float wv = fmaf(a.s, p[j], bf2f(old[j]));
                        uo[j] = f2bf(wv);
                        o[j] = f2bf(gelu_erf(wv));
                    }
                    if (arow && live) *(bf16x8*)(arow + n0 + c0) = uo;
                } else if (a.thr16 == 0) {                          // no dropout: c = drop_scale everywhere
                    o = lora_update8(a.sc, d0, d1, old);
                } else {
                    const uint32_t pair0 = (uint32_t)((flat + (uint64_t)(n0 + c0)) >> 1);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {                   // one hash word per element pair, decided on the packed halves
                        const uint32_t dm = mmb_drop_mask2(mmb_pair_bits(a.dstream, pair0 + q), a.thr_pk);
                        const bf16_t v0 = f2bf(fmaf(a.sc, p[2 * q], bf2f(old[2 * q])));
                        const bf16_t v1 = f2bf(fmaf(a.sc, p[2 * q + 1], bf2f(old[2 * q + 1])));
                        o[2 * q] = (dm & 0xFFFFu) ? old[2 * q] : v0;
                        o[2 * q + 1] = (dm >> 16) ? old[2 * q + 1] : v1;
                    }
                }
                if (live) *(bf16x8*)(yrow + n0 + c0) = o;
            }
        }
        __syncthreads();
    }
}

// backward launch 1: g (and h, when it is recomputed) into the workspace, and the in-place update of the input gradient
template <bool DROP>
__global__ __launch_bounds__(256) void lora_dense_bwd_g_kernel(const LoraDenseBwdArgs a) {
    __shared__ __attribute__((aligned(16))) bf16_t T[LORA_DTILE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
    const int K = a.K, N = a.N, r = a.r;
    const int m = blockIdx.x * LORA_ROWS + wave * 16 + (lane & 15);
    const bool live = m < a.M;
    const bool wave_live = blockIdx.x * LORA_ROWS + wave * 16 < a.M;
    const int mr = live ? m : a.M - 1;
    const uint32_t rowpair = DROP ? lora_row_pair(a.in.rows, mr, K) : 0u;   // the mask of the SITE row: rows[mr] on gathered operands
    if (a.recompute) {                                               // h = bf16(x . A^T), as forward formed it
        const bf16x4 hb = lora_round4(lora_dense_contract<DROP>(T, a.A, true, a.x + (size_t)mr * a.ldx, K, r, wave_live, lane, a.in, rowpair));
        if (live && 4 * g < r) *(bf16x4*)(a.hbuf + (size_t)m * r + 4 * g) = hb;
    }
    f32x4 gacc = lora_dense_contract<false>(T, a.B, false, a.dy + (size_t)mr * a.lddy, N, r, wave_live, lane, a.in, 0u);
    if constexpr (DROP) gacc *= a.in.c;                              // g carries c: dA and the input gradient need no further factor
    const bf16x4 gb = lora_round4(gacc);
    const bf16x8 gf = lora_low4(gb);
    if (live && 4 * g < r) *(bf16x4*)(a.gbuf + (size_t)m * r + 4 * g) = gb;
    if (!a.dx) return;                                               // (uniform over the grid)
    bf16_t* drow = a.dx + (size_t)mr * a.lddx + 8 * g;
    const bf16_t* urow = a.u ? a.u + (size_t)mr * a.ldu + 8 * g : nullptr;
    for (int k0 = 0; k0 < K; k0 += LORA_DCHUNK) {
        const int w = min(LORA_DCHUNK, K - k0);
        lora_stage_pad16_t(T, a.A, K, k0, w, r);
        __syncthreads();
        if (wave_live) {
            for (int c0 = 0; c0 < w; c0 += 32) {
                const bf16x8 old = *(const bf16x8*)(drow + k0 + c0);
                f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = {0.f, 0.f, 0.f, 0.f};
                lora_expand32(T, c0, gf, lane, d0, d1);
                if (urow) {                                          // the FFN-down seam: the base input gradient carries the same gelu' factor
                    const bf16x8 uv = *(const bf16x8*)(urow + k0 + c0);
#pragma unroll
                    for (int j = 0; j < 4; ++j) { d0[j] *= gelu_erf_grad(bf2f(uv[j])); d1[j] *= gelu_erf_grad(bf2f(uv[4 + j])); }
                }
                bf16x8 o = lora_update8(a.s, d0, d1, old);
                if constexpr (DROP) o = lora_keep_old8(o, old, a.in.stream, rowpair + (uint32_t)((k0 + c0 + 8 * g) >> 1), a.in.thr_pk);
                if (live) *(bf16x8*)(drow + k0 + c0) = o;
            }
        }
        __syncthreads();
    }
}

static inline bool lora_dense_shape_ok(int M, int K, int N, int r) {
    return M >= 0 && K > 0 && N > 0 && (K & 63) == 0 && (N & 63) == 0 && (r == 4 || r == 8 || r == 16);
}
// what ONE workgroup stages at a time; constant in K and N (the chunking), so the -2 of the convention cannot occur for these kernels
static inline size_t lora_dense_lds_bytes() { return (size_t)LORA_DTILE * sizeof(bf16_t); }

extern "C" {

static int lora_dense_fwd_impl(hipStream_t stream, const void* x, int ldx, void* y, int ldy, int M, int K, int N, int r, const void* A, const void* B,
                               float scale, int mode, unsigned drop_stream, unsigned drop_thr16, float drop_scale, void* aux, int ldaux,
                               void* h_out, int ldh, unsigned in_stream, unsigned in_thr16, float in_scale) {
    if (!lora_dense_shape_ok(M, K, N, r) || (mode != MMBERT_LORA_DENSE_ADD && mode != MMBERT_LORA_DENSE_GELU)) return -1;
    if (!lora_in_drop_ok(in_thr16, in_scale)) return -1;
    if (M == 0) return 0;
    if (!x || !y || !A || !B || !lora_al16(x) || !lora_al16(y) || !lora_al16(A) || !lora_al16(B)) return -1;
    if (ldx < K || (ldx & 7) || ldy < N || (ldy & 7) || drop_thr16 > 65535u) return -1;
    if (aux && (mode != MMBERT_LORA_DENSE_GELU || !lora_al16(aux) || ldaux < N || (ldaux & 7))) return -1;
    if (h_out && (!lora_al8(h_out) || ldh < r || (ldh & 3))) return -1;
    if (lora_dense_lds_bytes() > LORA_LDS_MAX) return -2;
    LoraDenseFwdArgs a = {};
    a.x = (const bf16_t*)x; a.y = (bf16_t*)y; a.A = (const bf16_t*)A; a.B = (const bf16_t*)B; a.aux = (bf16_t*)aux; a.h = (bf16_t*)h_out;
    a.M = M; a.K = K; a.N = N; a.r = r; a.ldx = ldx; a.ldy = ldy; a.ldaux = ldaux; a.ldh = ldh; a.gelu = mode == MMBERT_LORA_DENSE_GELU;
    a.s = scale; a.sc = scale * drop_scale;
    a.dstream = drop_stream; a.thr16 = a.gelu ? 0u : drop_thr16; a.thr_pk = mmb_thr_packed(drop_thr16);
    a.in = lora_in_drop(in_stream, in_thr16, in_scale, nullptr);
    return in_thr16 ? lora_rows_launch<lora_dense_fwd_kernel<true>>(stream, a, 0) : lora_rows_launch<lora_dense_fwd_kernel<false>>(stream, a, 0);
}

int mmbert_lora_dense_fwd(hipStream_t stream, const void* x, int ldx, void* y, int ldy, int M, int K, int N, int r, const void* A, const void* B,
                          float scale, int mode, unsigned drop_stream, unsigned drop_thr16, float drop_scale, void* aux, int ldaux,
                          void* h_out, int ldh) {
    return lora_dense_fwd_impl(stream, x, ldx, y, ldy, M, K, N, r, A, B, scale, mode, drop_stream, drop_thr16, drop_scale, aux, ldaux, h_out, ldh,
                               0u, 0u, 1.0f);
}

int mmbert_lora_dense_fwd_drop(hipStream_t stream, const void* x, int ldx, void* y, int ldy, int M, int K, int N, int r, const void* A, const void* B,
                               float scale, int mode, unsigned drop_stream, unsigned drop_thr16, float drop_scale, void* aux, int ldaux,
                               void* h_out, int ldh, unsigned in_stream, unsigned in_thr16, float in_scale) {
    return lora_dense_fwd_impl(stream, x, ldx, y, ldy, M, K, N, r, A, B, scale, mode, drop_stream, drop_thr16, drop_scale, aux, ldaux, h_out, ldh,
                               in_stream, in_thr16, in_scale);
}

// [partial sums: slabs x r (K + N) floats][g: M x r bf16][h, when backward recomputes it: the same]; 0 for M == 0 or a bad shape
size_t mmbert_lora_dense_bwd_workspace(int M, int K, int N, int r) {
    if (!lora_dense_shape_ok(M, K, N, r) || M == 0) return 0;
    const size_t nslab = (size_t)(M + LORA_SLAB - 1) / LORA_SLAB;
    const size_t part = nslab * (size_t)r * ((size_t)K + (size_t)N) * sizeof(float);
    const size_t gb = lora_up16((size_t)M * r * sizeof(bf16_t));
    return part + 2 * gb;
}

static int lora_dense_bwd_impl(hipStream_t stream, const void* dy, int lddy, const void* x, int ldx, const void* h, int ldh, int M, int K, int N, int r,
                               const void* A, const void* B, float scale, void* dx, int lddx, const void* gelu_u, int ldu, float* gA, float* gB,
                               int accumulate, void* workspace, unsigned in_stream, unsigned in_thr16, float in_scale, const int32_t* rows) {
    if (!lora_dense_shape_ok(M, K, N, r) || !lora_in_drop_ok(in_thr16, in_scale) || ((uintptr_t)rows & 3)) return -1;
    if (M == 0) return 0;
    if (!dy || !x || !A || !B || !lora_al16(dy) || !lora_al16(x) || !lora_al16(A) || !lora_al16(B)) return -1;
    if (lddy < N || (lddy & 7) || ldx < K || (ldx & 7)) return -1;
    if (h && (!lora_al8(h) || ldh < r || (ldh & 3))) return -1;
    if (dx && (!lora_al16(dx) || lddx < K || (lddx & 7))) return -1;
    if (gelu_u && (!dx || !lora_al16(gelu_u) || ldu < K || (ldu & 7))) return -1;
    if ((gA && !lora_al16(gA)) || (gB && !lora_al16(gB))) return -1;
    if (!workspace || !lora_al16(workspace)) return -3;
    if (lora_dense_lds_bytes() > LORA_LDS_MAX) return -2;
    if (!dx && !gA && !gB) return 0;                                 // nothing asked for
    const int nslab = (M + LORA_SLAB - 1) / LORA_SLAB;
    const size_t part = (size_t)nslab * (size_t)r * ((size_t)K + (size_t)N) * sizeof(float);
    const size_t gb = lora_up16((size_t)M * r * sizeof(bf16_t));
    LoraDenseBwdArgs a = {};
    a.dy = (const bf16_t*)dy; a.x = (const bf16_t*)x; a.A = (const bf16_t*)A; a.B = (const bf16_t*)B; a.u = (const bf16_t*)gelu_u; a.dx = (bf16_t*)dx;
    a.gbuf = (bf16_t*)((char*)workspace + part); a.hbuf = (bf16_t*)((char*)workspace + part + gb);
    a.M = M; a.K = K; a.N = N; a.r = r; a.lddy = lddy; a.ldx = ldx; a.lddx = lddx; a.ldu = ldu; a.s = scale;
    a.recompute = (gB && !h) ? 1 : 0;
    // the weight-gradient streams that run: dA needs g and x (width K), dB needs dy and h (width N)
    LoraWArgs w = {};
    int wmax = 0;
    if (gA) {
        LoraStream& s = w.st[w.ns++];
        s.src = a.x; s.lds = ldx; s.coef = a.gbuf; s.ldc = r; s.out = gA; s.colmajor = 0; s.acc = accumulate ? 1 : 0; s.W = K; s.part_off = 0;
        wmax = K;
    }
    if (gB) {
        LoraStream& s = w.st[w.ns++];
        s.src = a.dy; s.lds = lddy; s.out = gB; s.colmajor = 1; s.acc = accumulate ? 1 : 0; s.W = N; s.part_off = (size_t)nslab * (size_t)r * (size_t)K;
        if (h) { s.coef = (const bf16_t*)h; s.ldc = ldh; }
        else { s.coef = a.hbuf; s.ldc = r; }
        if (N > wmax) wmax = N;
    }
    a.in = w.in = lora_in_drop(in_stream, in_thr16, in_scale, rows);
    const int e = in_thr16 ? lora_rows_launch<lora_dense_bwd_g_kernel<true>>(stream, a, 0) : lora_rows_launch<lora_dense_bwd_g_kernel<false>>(stream, a, 0);
    if (e || w.ns == 0) return e;
    w.M = M; w.r = r; w.nslab = nslab; w.col_lanes = 128; w.s = scale; w.part = (float*)workspace;
    return in_thr16 ? lora_bwd_w_launch<true>(stream, w, wmax) : lora_bwd_w_launch<false>(stream, w, wmax);
}

int mmbert_lora_dense_bwd(hipStream_t stream, const void* dy, int lddy, const void* x, int ldx, const void* h, int ldh, int M, int K, int N, int r,
                          const void* A, const void* B, float scale, void* dx, int lddx, const void* gelu_u, int ldu, float* gA, float* gB,
                          int accumulate, void* workspace) {
    return lora_dense_bwd_impl(stream, dy, lddy, x, ldx, h, ldh, M, K, N, r, A, B, scale, dx, lddx, gelu_u, ldu, gA, gB, accumulate, workspace,
                               0u, 0u, 1.0f, nullptr);
}

int mmbert_lora_dense_bwd_drop(hipStream_t stream, const void* dy, int lddy, const void* x, int ldx, const void* h, int ldh, int M, int K, int N, int r,
                               const void* A, const void* B, float scale, void* dx, int lddx, const void* gelu_u, int ldu, float* gA, float* gB,
                               int accumulate, void* workspace, unsigned in_stream, unsigned in_thr16, float in_scale, const int* rows) {
    return lora_dense_bwd_impl(stream, dy, lddy, x, ldx, h, ldh, M, K, N, r, A, B, scale, dx, lddx, gelu_u, ldu, gA, gB, accumulate, workspace,
                               in_stream, in_thr16, in_scale, (const int32_t*)rows);
}

}  // extern "C"
