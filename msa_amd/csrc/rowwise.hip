// HBM-bound row-wise kernels of the MMBert train step (gfx950): embedding gather / scatter-add, the JointEmbeddings
// pair projection (K = 35/74/47/371/81: far too thin for MFMA, plain FMA), vocabulary
// cross-entropy over bf16 logits, the flat AdamW update (+ bf16 weight refresh), and the batched
// fp32 -> bf16 transpose that maintains the dgrad weight copies.  (The LayerNorm kernels: layernorm.hip.)
//
// Conventions: one wave (64 lanes) per row, 8-byte bf16x4 accesses, fp32 statistics, row-index
// maps (int32) where a kernel gathers or scatters rows of the packed token matrix.
#include "common.h"
#include "../../include/mmbert_hip.h"
#include <cstring>

std::atomic<int> g_mmb_deterministic{0};     // mmbert_set_deterministic (common.h: every translation unit of the library reads it)

// Row maps of the valid-first packing (ops.SplitLayout): packed row of every original row (inv) and back (perm), from the
// per-sequence unmasked length `valid`, the region starts and the row -> (sequence, position) tables.  mode 0: masked-out rows
// go to region B in order; 1: all masked-out rows of a sequence share its ONE region-B row (inference); 2: they are left out
// (inv = rows_a, one past the packed matrix).
// ``rank`` (optional, mmbert_prologue's row-set mode): the position of every row in its sequence's OWN valid-first order (active
// rows first, order kept) -- it replaces row_pos, so that the leading ``valid[s]`` rows of sequence s are its active rows wherever
// they sit in the original sequence (the fused text | visual | speech sequence has its visual padding in the middle).
__global__ void split_rows_kernel(const int64_t* __restrict__ row_seq, const int64_t* __restrict__ row_pos, const int* __restrict__ start_a,
                                  const int* __restrict__ start_b, const int* __restrict__ valid, int mode, int M, int rows_a,
                                  int64_t* __restrict__ perm, int64_t* __restrict__ inv, const int* __restrict__ rank,
                                  int* __restrict__ perm32, int* __restrict__ inv32) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const int s = (int)row_seq[i], p = rank ? rank[i] : (int)row_pos[i], v = valid[s];
    int n = rows_a;
    bool own = false;                                          // does packed row n stand for original row i?
    if (p < v) { n = start_a[s] + p; own = true; }
    else if (mode == 0) { n = start_b[s] + p - v; own = true; }
    else if (mode == 1) { n = start_b[s]; own = p == v; }
    inv[i] = n;
    if (inv32) inv32[i] = n;
    if (own) { perm[n] = i; if (perm32) perm32[n] = i; }
}

// The valid-first packing's per-sequence starts and attention tile lists, built on the DEVICE from the prologue's ``valid`` counts
// (round 3; ops.SplitLayout's numpy form needs them on the host: one blocking round trip per forward pass).  One workgroup:
//   v[s] = min(valid[s], len[s]);  start_a = exclusive prefix sum of v;  start_b = rows_a + exclusive prefix sum of (len - v);
//   region-A tiles (s, k), k < ceil(v / rows), then region-B tiles (s, k), k < ceil((len - v) / rows) -- each list ordered
//   longest-work-first with the sequences interleaved in groups of xs (ops.SplitLayout's rule: rank = stable order of -v; key =
//   (rank / xs, k, rank % xs));
//   unused list entries (the lists are sized for the worst case) get sequence -1: the attention kernels leave at once.
// out (int32): ftile_seq | ftile_r0 | ftile_qshift | ftile_qend  (nf_max each)  |  tile_seq | tile_r0 | qtile_qshift | qtile_qend
// (nq_max each)  |  start_a | v | start_b (nseq each)  |  counts: nf, nq, rows_a, 0.
#define SL_MAXSEQ 1024
__global__ __launch_bounds__(1024) void split_layout_kernel(const int* __restrict__ lens, const int* __restrict__ valid, int nseq, int rows, int xs,
                                                            int nf_max, int nq_max, int* __restrict__ out) {
    __shared__ int v[SL_MAXSEQ], ln[SL_MAXSEQ], rk[SL_MAXSEQ], sa[SL_MAXSEQ], sb[SL_MAXSEQ], seq_of_rank[SL_MAXSEQ], ntr[SL_MAXSEQ];
    __shared__ int tot[3];
    const int tid = threadIdx.x;
    if (tid < 3) tot[tid] = 0;
    for (int s = tid; s < nseq; s += 1024) { ln[s] = lens[s]; v[s] = min(valid[s], lens[s]); }
    __syncthreads();
    // Every sequence's thread walks the others itself -- stable rank of -v and both exclusive prefix sums in one pass of independent
    // LDS reads.  (Thread 0 alone used to run the two prefix sums and the two tile totals as dependent LDS chains: 4 x nseq steps
    // of a read-add-write each, most of the kernel's 23 us in front of every forward pass.)
    for (int s = tid; s < nseq; s += 1024) {
        int r = 0, a = 0, b = 0;
        const int vs = v[s];
        for (int t = 0; t < nseq; ++t) {
            const int vt = v[t];
            r += (vt > vs || (vt == vs && t < s)) ? 1 : 0;
            if (t < s) { a += vt; b += ln[t] - vt; }
        }
        rk[s] = r;
        seq_of_rank[r] = s;
        sa[s] = a; sb[s] = b;
        if (s == nseq - 1) tot[2] = a + vs;
    }
    __syncthreads();
    for (int s = tid; s < nseq; s += 1024) sb[s] += tot[2];
    __syncthreads();
    int* f_seq = out; int* f_r0 = out + nf_max; int* f_sh = out + 2 * nf_max; int* f_end = out + 3 * nf_max;
    int* q_seq = out + 4 * nf_max; int* q_r0 = q_seq + nq_max; int* q_sh = q_seq + 2 * nq_max; int* q_end = q_seq + 3 * nq_max;
    int* o_sa = q_seq + 4 * nq_max; int* o_v = o_sa + nseq; int* o_sb = o_v + nseq; int* o_cnt = o_sb + nseq;
    for (int s = tid; s < nseq; s += 1024) { o_sa[s] = sa[s]; o_v[s] = v[s]; o_sb[s] = sb[s]; }
    // position of tile (s, k) of a list with nt[.] tiles per sequence: tiles of earlier groups, then inside the group by (k, rank % xs)
    auto place = [&](bool regionB, int base, int* cnt_out) {
        auto nt = [&](int s) { const int c = regionB ? ln[s] - v[s] : v[s]; return (c + rows - 1) / rows; };
        for (int s = tid; s < nseq; s += 1024) {                 // tiles per sequence in RANK order (one division per sequence), and their total
            const int n = nt(s);
            ntr[rk[s]] = n;
            if (n) atomicAdd(cnt_out, n);
        }
        __syncthreads();
        for (int s = tid; s < nseq; s += 1024) {
            const int r = rk[s], n = ntr[r];
            if (n == 0) continue;
            const int g = r / xs, m = r - g * xs;
            int before_groups = 0;
            for (int r2 = 0; r2 < g * xs; ++r2) before_groups += ntr[r2];
            for (int k = 0; k < n; ++k) {
                int pos = before_groups;
                for (int m2 = 0; m2 < xs && g * xs + m2 < nseq; ++m2) {
                    const int n2 = ntr[g * xs + m2];
                    pos += min(n2, k) + ((n2 > k && m2 < m) ? 1 : 0);
                }
                const int first = regionB ? v[s] : 0, shift = regionB ? sb[s] - v[s] : sa[s], end = regionB ? ln[s] : v[s];
                f_seq[base + pos] = s; f_r0[base + pos] = first + k * rows; f_sh[base + pos] = shift; f_end[base + pos] = end;
                if (!regionB) { q_seq[pos] = s; q_r0[pos] = k * rows; q_sh[pos] = shift; q_end[pos] = end; }
            }
        }
        __syncthreads();                                          // (ntr is rewritten by the next region; the total is complete)
    };
    place(false, 0, &tot[0]);
    __syncthreads();
    const int nA = tot[0];
    place(true, nA, &tot[1]);
    __syncthreads();
    const int nf = nA + tot[1];
    for (int i = nf + tid; i < nf_max; i += 1024) { f_seq[i] = -1; f_r0[i] = 0; f_sh[i] = 0; f_end[i] = 0; }
    for (int i = nA + tid; i < nq_max; i += 1024) { q_seq[i] = -1; q_r0[i] = 0; q_sh[i] = 0; q_end[i] = 0; }
    if (tid == 0) { o_cnt[0] = nf; o_cnt[1] = nA; o_cnt[2] = tot[2]; o_cnt[3] = 0; }
}

// --------------------------------------------------------------------------------------------
// Embedding gather: out[i] = word[ids[i]] + type[tt[i]] + pos[i % T]      (fp32 tables -> bf16)
// --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void embed_gather_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ tts,
                                                           const float* __restrict__ word, const float* __restrict__ type,
                                                           const float* __restrict__ pos, int n, int T, int H, int V,
                                                           bf16_t* __restrict__ out, int ldo) {
    const int lane = threadIdx.x & 63;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += gridDim.x * 4) {
        long id = ids[i]; if (id < 0 || id >= V) id = 0;
        const long tt = tts ? (tts[i] != 0) : 0;
        const float* wr = word + (size_t)id * H;
        const float* tr = type + (size_t)tt * H;
        const float* pr = pos + (size_t)(i % T) * H;
        for (int col = lane * 4; col < H; col += 256) {
            const float4 a = *(const float4*)(wr + col), b = *(const float4*)(tr + col), c = *(const float4*)(pr + col);
            bf16x4 o = {f2bf(a.x + b.x + c.x), f2bf(a.y + b.y + c.y), f2bf(a.z + b.z + c.z), f2bf(a.w + b.w + c.w)};
            *(bf16x4*)(out + (size_t)i * ldo + col) = o;
        }
    }
}

// scatter-add of d(embedding sum): word rows (not row 0: padding_idx), position rows, and the two token-type rows.
// One workgroup per POSITION p (rows p, p + T, p + 2T, ...: the same position of every sequence), a thread owns 4 columns: the
// position row and the token-type rows are summed in registers over the sequences and leave as one add per column (the first
// form gave every row its own atomics: 48 sequences contending for each of the T position rows, 75 us at 2400 rows); only the
// word rows, which rarely collide, take an atomic per row.
__global__ __launch_bounds__(256) void embed_scatter_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ tts,
                                                            const bf16_t* __restrict__ d, int ldd, int n, int T, int H, int V,
                                                            float* __restrict__ gword, float* __restrict__ gtype, float* __restrict__ gpos,
                                                            float* __restrict__ type_slab) {
    // type_slab (deterministic mode, one slice): the position's two token-type sums are STORED to type_slab[p][0 / 1][col] and folded in
    // position order by embed_type_fold_kernel, instead of T workgroups adding to the same two rows in arrival order.
    // (round 4) The loop over the sequences was one dependent memory round trip per row (id -> branch -> atomics: 47 us for 48 rows per
    // workgroup, on the critical path in front of the optimizer): the rows now come in BATCHES of 8 whose loads are issued together, and
    // blockIdx.y takes every gridDim.y-th batch -- one slice by default: more slices LOSE (every slice adds its token-type sums to the
    // same two rows: T x slices same-address atomics per element; 8 slices with a row per trip: 85 us), the rest is the word rows' atomics.
    const int p = blockIdx.x;
    for (int col = threadIdx.x * 4; col < H; col += 1024) {
        float ps[4] = {0.f, 0.f, 0.f, 0.f}, t0[4] = {0.f, 0.f, 0.f, 0.f}, t1[4] = {0.f, 0.f, 0.f, 0.f};
        for (int i0 = p + (int)blockIdx.y * 8 * T; i0 < n; i0 += 8 * T * (int)gridDim.y) {
            long id[8]; bool tt[8]; bf16x4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = min(i0 + u * T, n - 1);              // (clamped: a row past the end is loaded and not used)
                id[u] = ids[i];
                tt[u] = tts ? (tts[i] != 0) : false;
                v[u] = *(const bf16x4*)(d + (size_t)i * ldd + col);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (i0 + u * T >= n) break;
                const bool word = gword != nullptr && id[u] > 0 && id[u] < V;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float f = bf2f(v[u][r]);
                    ps[r] += f;
                    if (tt[u]) t1[r] += f; else t0[r] += f;
                    if (word) atomicAdd(gword + (size_t)id[u] * H + col + r, f);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            atomicAdd(gpos + (size_t)p * H + col + r, ps[r]);       // (one slice: the only adder of this address)
            if (type_slab) { type_slab[((size_t)p * 2) * H + col + r] = t0[r]; type_slab[((size_t)p * 2 + 1) * H + col + r] = t1[r]; }
            else {
                if (t0[r] != 0.f) atomicAdd(gtype + col + r, t0[r]);
                if (t1[r] != 0.f) atomicAdd(gtype + H + col + r, t1[r]);
            }
        }
    }
}

// --------------------------------------------------------------------------------------------
// JointEmbeddings pair projection: out[out_row0 + b*(T+P) + T + p] = relu(W . feat[b,p] + bias)
// feat fp32 [B*P, D]; W fp32 [H, D].
// --------------------------------------------------------------------------------------------
// On the fp32 MFMA (v_mfma_f32_16x16x4_f32: exact fp32 products summed as an fmaf chain over ascending k, as the scalar kernels
// before it summed): one workgroup = 128 hidden columns x 64 feature rows, 4 waves of 64 x 32 (4 x 2 MFMA tiles),
// M = hidden column, N = feature row, so that a lane ends with 4 consecutive columns of one row.  Both operand tiles are copied to LDS
// as they lie in memory (row-major, k padded to a multiple of 4 with zeros; row pitch = 2 mod 16 floats: the 16 rows x 2 k of a
// half-wave's ds_read_b32 fall in 32 different banks).  D beyond 128 runs in chunks of 128.  The sums are fmaf chains over ascending k.
// (Round 1: 16 rows per workgroup, every thread streaming its own W row from global memory, 27 / 54 us for D = 35 / 74 at 8000 rows;
// round 2: 64 x 64 tile with scalar LDS reads, 28 / 43 us; round 4: 128 x 64 tile, K-major LDS, three ds_read_b128 per 32 FMAs,
// 23 / 35 us stand-alone, 30 / 43 us in the step's trace, against a scalar-FMA floor of 5.5 / 11.6 us; this form: 15 / 25 us by
// rocprofv3 (tools/r4_s3_pairprof.sh, profiles/r4_pair_proj.log).)
// FT = float, or double: the reference's collate hands the pair features over as float64 (REF:model_utils.py:94-99) and casts them in
// JointEmbeddings.forward (REF:MMBertEmbedding.py:62,64: `.float()`): read as they are and rounded on load, the cast launches are gone.
template <int KSHIFT, typename FT>
__global__ __launch_bounds__(256) void pair_proj_fwd_kernel(const FT* __restrict__ feat, int n_rows, int P, int D,
                                                            const float* __restrict__ W, const float* __restrict__ bias, int H,
                                                            bf16_t* __restrict__ out, int ldo, int T, int KC, int pitch) {
#if defined(__gfx950__)
    extern __shared__ __attribute__((aligned(16))) float pair_sm[];
    float* Ws = pair_sm;                         // [128][pitch]
    float* Fs = pair_sm + 128 * pitch;           // [64][pitch]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int row0 = blockIdx.x * 64, h0 = blockIdx.y * 128;
    const int wh = (wave & 1) * 64, wr = (wave >> 1) * 32;
    f32x4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // the bias of the lane's 16 columns, fetched first (clamped in range; unused past H): its latency passes under the staging
    float bcol[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) bcol[i][q] = bias[min(h0 + wh + 16 * i + 4 * g + q, H - 1)];
    // staging: a wave copies whole rows, lane = k (64 or 128 lanes of k per row), up to 32 rows in flight per wave (batches of 8 were
    // a memory round trip each).  Per-lane 32-bit offsets on the two base pointers: with wave-uniform row pointers hipcc runs out of
    // SGPRs, parks them in VGPR lanes and ends up waiting for every load before it issues the next (48 round trips, 20 us)
    constexpr int kw = 1 << KSHIFT, rstep = 256 >> KSHIFT;
    const int kl = tid & (kw - 1), rsub = tid >> KSHIFT;
    for (int k0 = 0; k0 < D; k0 += KC) {
        const int kc = min(KC, D - k0), kc4 = (kc + 3) & ~3;
        if (k0) __syncthreads();
        const float kmask = kl < kc ? 1.f : 0.f;
        const int kg = min(k0 + kl, D - 1);                             // always in range: the load is not predicated (a product, not a
        const bool kst = kl < kc4;                                       // select, zeroes the padding: see pair_wgrad_kernel)
        auto stage = [&](auto base, int g0, int lim, int lrow0, auto nrows_c) {
            constexpr int N = decltype(nrows_c)::value / rstep, NB = N < 32 ? N : 32;
#pragma unroll 1
            for (int ub = 0; ub < N; ub += NB) {
                std::remove_cv_t<std::remove_reference_t<decltype(base[0])>> v[NB];       // (float, or double: converted behind the last load)
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const int gr = g0 + rsub + (ub + u) * rstep;
                    v[u] = base[(uint32_t)(min(gr, lim - 1) * D + kg)];
                }
                if (kst) {
#pragma unroll
                    for (int u = 0; u < NB; ++u) {
                        const int r = rsub + (ub + u) * rstep;
                        pair_sm[(lrow0 + r) * pitch + kl] = (float)v[u] * (g0 + r < lim ? kmask : 0.f);
                    }
                }
            }
        };
        stage(W, h0, H, 0, std::integral_constant<int, 128>{});
        stage(feat, row0, n_rows, 128, std::integral_constant<int, 64>{});
        __syncthreads();
        const float* wa = Ws + (wh + c) * pitch + g;
        const float* fb = Fs + (wr + c) * pitch + g;
        float av[4], bv[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) av[i] = wa[16 * i * pitch];
#pragma unroll
        for (int j = 0; j < 2; ++j) bv[j] = fb[16 * j * pitch];
        for (int kk = 0; kk < kc4; kk += 4) {
            float an[4], bn[2];
            const int kn = kk + 4 < kc4 ? kk + 4 : kk;                  // the next step's fragments are read under this step's MFMAs
#pragma unroll
            for (int i = 0; i < 4; ++i) an[i] = wa[16 * i * pitch + kn];
#pragma unroll
            for (int j = 0; j < 2; ++j) bn[j] = fb[16 * j * pitch + kn];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 4; ++i) av[i] = an[i];
#pragma unroll
            for (int j = 0; j < 2; ++j) bv[j] = bn[j];
        }
    }
    // acc[i][j][q] = column h0 + wh + 16 i + 4 g + q of row row0 + wr + 16 j + c.  Stored from there a wave-instruction is 16 rows x 32
    // bytes, and the kernel is bound by issuing those (20 us at 8000 rows whatever D); so the tile goes through LDS (bf16, [64][128 + 8])
    // and leaves as whole 256-byte rows, 16 bytes per lane
    if (h0 + 128 <= H && !(ldo & 7)) {
        __syncthreads();
        bf16_t* Os = (bf16_t*)pair_sm;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                bf16x4 ov = {f2bf(fmaxf(acc[i][j][0] + bcol[i][0], 0.f)), f2bf(fmaxf(acc[i][j][1] + bcol[i][1], 0.f)),
                             f2bf(fmaxf(acc[i][j][2] + bcol[i][2], 0.f)), f2bf(fmaxf(acc[i][j][3] + bcol[i][3], 0.f))};
                *(bf16x4*)(Os + (wr + 16 * j + c) * 136 + wh + 16 * i + 4 * g) = ov;
            }
        __syncthreads();
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) {
            const int rl = (tid >> 4) + 16 * ps, row = row0 + rl;
            if (row >= n_rows) continue;
            const int b_ = row / P, p_ = row - b_ * P;
            *(bf16x8*)(out + (size_t)(b_ * (T + P) + T + p_) * ldo + h0 + 8 * (tid & 15)) = *(const bf16x8*)(Os + rl * 136 + 8 * (tid & 15));
        }
        return;
    }
    // acc[i][j][q] = column h0 + wh + 16 i + 4 g + q of row row0 + wr + 16 j + c
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int row = row0 + wr + 16 * j + c;
        if (row >= n_rows) continue;
        const int b_ = row / P, p_ = row - b_ * P;
        bf16_t* orow = out + (size_t)(b_ * (T + P) + T + p_) * ldo;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int h = h0 + wh + 16 * i + 4 * g;
            if (h + 3 < H && !(ldo & 3)) {
                bf16x4 ov = {f2bf(fmaxf(acc[i][j][0] + bcol[i][0], 0.f)), f2bf(fmaxf(acc[i][j][1] + bcol[i][1], 0.f)),
                             f2bf(fmaxf(acc[i][j][2] + bcol[i][2], 0.f)), f2bf(fmaxf(acc[i][j][3] + bcol[i][3], 0.f))};
                *(bf16x4*)(orow + h) = ov;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) if (h + q < H) orow[h + q] = f2bf(fmaxf(acc[i][j][q] + bcol[i][q], 0.f));
            }
        }
    }
#endif
}

// backward: dpre = dJ * (J > 0); dW[h][k] += sum_rows dpre[row][h]*feat[row][k]; db[h] += sum_rows dpre[row][h].
// A tokens-contracted product with a tiny output ([H, D], D = 35 / 74) and fp32 features: it runs on the fp32 MFMA
// (v_mfma_f32_16x16x4_f32: exact fp32 products, an fmaf chain over the rows), operands straight from global memory in fragment order:
//   * contraction = rows, 4 per MFMA (lane group g = lane >> 4 holds row r + g); M = 16 hidden columns, N = 16 feature columns;
//   * the A fragment of M-tile i takes column hb + 4 m + i from lane m, so ONE 8-byte load per lane of J and of dJ (columns
//     hb + 4 m .. + 3 of its row: 128 contiguous bytes per row and instruction) feeds the four M-tiles of a wave's 64 columns;
//   * feature column D is the constant 1: the bias gradient is column D of the product, no separate column sum;
//   * a workgroup = 64 hidden columns x one range of rows, its 4 waves a quarter of the range each, summed through LDS in wave order;
//     the per-range partial tiles go to a slab [S][H][D + 1] and pair_wgrad_reduce_kernel adds them to dW / db in range order
//     (deterministic: no atomics).
// (Round 1: a scalar-FMA kernel with one atomicAdd per weight and row chunk, 300 us for D = 74 at 8000 rows; rounds 2-4: a bf16 hi / lo
// split of the features through the grouped TN kernel, four launches and 49 us; this form: two launches, 26 + 4.5 us.)
struct PairBwdArgs { const void* feat; const bf16_t* J; const bf16_t* dJ; float* slab; int n, P, D, T, H, ld, rows_per_wg, ntiles; };
constexpr int PAIR_NT = 5;                       // feature-column tiles (16 columns) per workgroup: D + 1 <= 80 in one pass, more on grid.z

template <typename FT>
__global__ __launch_bounds__(256) void pair_wgrad_kernel(const PairBwdArgs a) {
#if defined(__gfx950__)
    __shared__ float red[3][PAIR_NT * 16][64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int hb = blockIdx.x * 64, s = blockIdx.y, jt0 = blockIdx.z * PAIR_NT;
    const int njt = min(PAIR_NT, a.ntiles - jt0);
    const int rpw = a.rows_per_wg >> 2;                                  // rows per wave: a multiple of 16
    const int r0 = s * a.rows_per_wg + wave * rpw, r1 = min(r0 + rpw, a.n);
    const int hcol = hb + 4 * c;
    const bool hok = hcol + 3 < a.H;
    struct Stage { bf16x4 j, d; float f[PAIR_NT]; };
    auto load = [&](Stage& st, int r) {
        const bool ok = r < r1;
        const int rc = ok ? r : 0;
        const int b_ = rc / a.P, p_ = rc - b_ * a.P;
        const size_t off = (size_t)(b_ * (a.T + a.P) + a.T + p_) * a.ld + (hok ? hcol : 0);
        st.j = *(const bf16x4*)(a.J + off);
        st.d = *(const bf16x4*)(a.dJ + off);
        const FT* fr = (const FT*)a.feat + (size_t)rc * a.D;
#pragma unroll
        for (int j = 0; j < PAIR_NT; ++j) {
            const int k = (jt0 + j) * 16 + c;
            // (arithmetic, not a select, on the loaded value: hipcc sinks a load whose only use is one arm of a select into a branch
            // of its own, and every such branch ends in s_waitcnt vmcnt(0) -- the ring would hold one load at a time)
            const float live = (ok && j < njt) ? 1.0f : 0.0f;
            st.f[j] = fmaf((float)fr[min(k, a.D - 1)], k < a.D ? live : 0.0f, k == a.D ? live : 0.0f);
        }
        if (!(ok && hok)) { st.d = (bf16x4){(bf16_t)0.0f, (bf16_t)0.0f, (bf16_t)0.0f, (bf16_t)0.0f}; }
    };
    f32x4 acc[PAIR_NT][4];
#pragma unroll
    for (int j = 0; j < PAIR_NT; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // four steps of 4 rows in flight per wave (one wave per SIMD: nothing else hides the memory latency); the ring is unrolled so
    // that a stage is refilled in place -- rotating it through register copies would wait for the newest load in every step.
    // (hipcc still moves a stage's loads from the end of one turn to the top of the next; inline-asm loads behind counted waits ran
    // 21 instead of 26 us, and with eight stages the register allocator copied an asm output before its wait: the load landed in a
    // register that by then held an address -- a memory fault.  Asynchronous asm outputs are not worth 5 us: plain loads stay.)
    Stage st[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) load(st[u], r0 + 4 * u + g);
#pragma unroll 1
    for (int r = r0; r < r1; r += 16) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float av[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) av[i] = bf2f(st[u].j[i]) > 0.f ? bf2f(st[u].d[i]) : 0.f;
            float fv[PAIR_NT];
#pragma unroll
            for (int j = 0; j < PAIR_NT; ++j) fv[j] = st[u].f[j];
            load(st[u], r + 16 + 4 * u + g);
#pragma unroll
            for (int j = 0; j < PAIR_NT; ++j) {
                if (j >= njt) continue;                               // (wave-uniform: D = 35 has three column tiles, not five)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], fv[j], acc[j][i], 0, 0, 0);
            }
        }
    }
    // waves 1-3 hand their tiles to wave 0, which adds them in wave order and writes the workgroup's partial product
    if (wave) {
#pragma unroll
        for (int j = 0; j < PAIR_NT; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) red[wave - 1][(j * 4 + i) * 4 + q][lane] = acc[j][i][q];
    }
    __syncthreads();
    if (wave == 0) {
        const int W1 = a.D + 1;
        float* out = a.slab + (size_t)s * a.H * W1;
#pragma unroll
        for (int j = 0; j < PAIR_NT; ++j) {
            const int k = (jt0 + j) * 16 + c;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int e = (j * 4 + i) * 4 + q;
                    const float v = ((acc[j][i][q] + red[0][e][lane]) + red[1][e][lane]) + red[2][e][lane];
                    const int h = hb + 4 * (4 * g + q) + i;              // D tile: row m = 4 g + q of M-tile i is column hb + 4 m + i
                    if (j < njt && k < W1 && h < a.H) out[(size_t)h * W1 + k] = v;
                }
        }
    }
#endif
}

// dW[h][k] += sum_s slab[s][h][k] (k < D), db[h] += sum_s slab[s][h][D], ranges in ascending order
__global__ void pair_wgrad_reduce_kernel(const float* __restrict__ slab, int S, int H, int D, float* __restrict__ dW, float* __restrict__ db) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int W1 = D + 1;
    if (i >= H * W1) return;
    float t = 0.f;
    int s_ = 0;
    for (; s_ + 8 <= S; s_ += 8) {                                     // eight loads in flight, added in range order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = slab[(size_t)(s_ + u) * H * W1 + i];
#pragma unroll
        for (int u = 0; u < 8; ++u) t += v[u];
    }
    for (; s_ < S; ++s_) t += slab[(size_t)s_ * H * W1 + i];
    const int h = i / W1, k = i - h * W1;
    if (k < D) dW[(size_t)h * D + k] += t; else db[h] += t;
}

// --------------------------------------------------------------------------------------------
// Vocabulary cross-entropy over bf16 logits [M, ldv] (first V columns valid), ignore_index -100.
// Rows are grouped into up to 4 segments (the text / text+visual / text+speech passes): each
// segment's loss is a mean over ITS non-ignored rows (REF get_outputs, one CrossEntropyLoss per pass).
//   ce_count : inv_count[s] = 1/max(1,#valid rows in segment s); loss_sum[s] = 0
//   ce_row<0>: forward  (loss per segment, per-row logsumexp kept for backward)
//   ce_row<1>: backward (dlogits, the upstream gradient of each segment's loss folded in, so the two
//              vocabulary GEMMs of backward run once over all rows instead of once per pass)
// --------------------------------------------------------------------------------------------
// Compact list of the rows that carry a label (0 <= label < V), in row order, plus their count: one workgroup, block scan.
// The MLM head's backward runs on these rows only: every other row of dlogits is exactly zero (ignore_index), so the two
// vocabulary-sized products, LayerNorm', GELU' and the transform products of backward need ~2 % of the rows.
__global__ __launch_bounds__(1024) void active_rows_kernel(const int64_t* __restrict__ labels, int M, int V, int* __restrict__ idx, int* __restrict__ count) {
    __shared__ int wsum[16];
    __shared__ int base;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < M; i0 += 1024) {
        const int i = i0 + tid;
        const bool act = i < M && labels[i] >= 0 && labels[i] < V;
        const unsigned long long bal = __ballot(act);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[w] = __popcll(bal);
        __syncthreads();
        int off = base;
        for (int q = 0; q < w; ++q) off += wsum[q];
        if (act) idx[off + before] = i;
        __syncthreads();
        if (tid == 0) { int t = 0; for (int q = 0; q < 16; ++q) t += wsum[q]; base += t; }
        __syncthreads();
    }
    if (tid == 0) *count = base;
}

// One predicate for "row i carries a label" in every kernel of the MLM head (ce_count / ce_row / active_rows): 0 <= label < V.
// -100 is the reference's ignore_index; any other value outside the vocabulary makes torch's CrossEntropyLoss raise in the
// reference -- here the host side counts such labels (model.mlm_active_rows) and raises when it reads the count.
__global__ void ce_count_kernel(const int64_t* __restrict__ labels, int M, int V, const int* __restrict__ seg_bounds, int nseg,
                                float* __restrict__ inv_count, float* __restrict__ loss_sum) {
    __shared__ int cnt[4];
    if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
    __syncthreads();
    // eight labels per thread in flight, counted in registers (one label at a time, with the segment search reading seg_bounds behind
    // each, the single workgroup made 18 dependent round trips at the headline size: 12 us in front of the loss)
    const int b1 = nseg > 1 ? seg_bounds[1] : 0x7fffffff, b2 = nseg > 2 ? seg_bounds[2] : 0x7fffffff, b3 = nseg > 3 ? seg_bounds[3] : 0x7fffffff;
    int c[4] = {0, 0, 0, 0};
    for (int i0 = threadIdx.x; i0 < M; i0 += (int)blockDim.x * 8) {
        int64_t lab[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) lab[u] = labels[min(i0 + u * (int)blockDim.x, M - 1)];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u * (int)blockDim.x;
            const int ok = (i < M && lab[u] >= 0 && lab[u] < V) ? 1 : 0;
            const int sg = (i >= b1 ? 1 : 0) + (i >= b2 ? 1 : 0) + (i >= b3 ? 1 : 0);
#pragma unroll
            for (int q = 0; q < 4; ++q) c[q] += (sg == q) ? ok : 0;
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) if (c[q]) atomicAdd(&cnt[q], c[q]);
    __syncthreads();
    if (threadIdx.x < nseg) {
        inv_count[threadIdx.x] = 1.0f / (float)max(cnt[threadIdx.x], 1);
        // torch CrossEntropyLoss(mean) over zero valid rows gives nan; the reference never hits it
        loss_sum[threadIdx.x] = 0.f;
    }
}

// Deterministic mode: loss_sum[seg] = the sum of the rows' loss terms (ce_row_kernel left them in row_loss, 0 for unlabelled rows) in a FIXED
// order -- thread t takes rows t, t + 1024, ... ascending, then a fixed-shape tree over the 1024 partial sums -- instead of one atomic per
// row in arrival order.
__global__ __launch_bounds__(1024) void ce_loss_sum_ordered_kernel(const float* __restrict__ row_loss, int M, const int* __restrict__ seg_bounds, int nseg,
                                                                   float* __restrict__ loss_sum) {
    __shared__ float red[4][1024];
    const int b1 = nseg > 1 ? seg_bounds[1] : 0x7fffffff, b2 = nseg > 2 ? seg_bounds[2] : 0x7fffffff, b3 = nseg > 3 ? seg_bounds[3] : 0x7fffffff;
    float c[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i0 = threadIdx.x; i0 < M; i0 += 1024 * 8) {            // eight rows per thread and trip: their loads go out together
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = row_loss[min(i0 + u * 1024, M - 1)];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u * 1024;
            const int sg = (i >= b1 ? 1 : 0) + (i >= b2 ? 1 : 0) + (i >= b3 ? 1 : 0);
            const float x = i < M ? v[u] : 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) c[q] += (sg == q) ? x : 0.f;
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) red[q][threadIdx.x] = c[q];
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
#pragma unroll
            for (int q = 0; q < 4; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + w];
        }
        __syncthreads();
    }
    if ((int)threadIdx.x < nseg) loss_sum[threadIdx.x] = red[threadIdx.x][0];
}

// Deterministic scatter-add of rows keyed by an id: dst[row_of(id)][:] += sum of src[i][:] over all rows i that carry that id, added in a
// FIXED association -- row group g (of G = blockDim / (H / 4)) sums the id's rows number g, g + G, ... (ascending i), then the G partial
// sums are added in the order g = 0 .. G - 1 -- with exactly one add per destination element, whatever the scheduling.  One workgroup
// per row i: it scans all n ids (a few KB, L2-resident), leaves at once unless i is the FIRST row of its id, and otherwise collects the
// id's rows in ascending order in LDS (wave 0, ballot compaction) and sums them.  No sort, no compaction on the host, nothing read back.
// row_of(id) = id (uni == null: the word-embedding table) or the id's index in the ascending list `uni` (the data-parallel row block);
// ids outside (0, V) or not in the list are skipped.  n <= 8192 (the LDS list).  Replaces the atomics of mmbert_embed_scatter's word rows
// and of mmbert_rows_to_block in deterministic mode.
#define RUNS_MAXN 8192
__global__ __launch_bounds__(1024) void id_runs_sum_rows_kernel(const void* __restrict__ src, int src_bf16, int lds, const int64_t* __restrict__ ids,
                                                                int n, int H, int V, const int64_t* __restrict__ uni, int U,
                                                                float* __restrict__ dst, int ldd) {
    __shared__ int list[RUNS_MAXN];
    __shared__ float red[1024 * 4];
    __shared__ int s_count, s_earlier;
    const int i0 = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const long long key = ids[i0];
    if (key <= 0 || key >= V) return;
    if (tid == 0) { s_count = 0; s_earlier = 0; }
    __syncthreads();
    int earlier = 0;
    for (int j = tid; j < i0; j += nthr) earlier |= (ids[j] == key) ? 1 : 0;
    if (earlier) s_earlier = 1;                                    // (benign: every writer stores 1)
    __syncthreads();
    if (s_earlier) return;
    long long dr = key;
    if (uni) {
        int lo = 0, hi = U - 1;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (uni[mid] < key) lo = mid + 1; else hi = mid; }
        if (U <= 0 || uni[lo] != key) return;
        dr = lo;
    }
    if (tid < 64) {                                                // wave 0: the id's rows from i0 on, ascending, into the list
        int count = 0;
        for (int base = i0; base < n; base += 64) {
            const int j = base + tid;
            const bool hit = j < n && ids[j] == key;
            const unsigned long long m = __ballot(hit);
            if (hit) list[count + __popcll(m & ((1ull << tid) - 1ull))] = j;
            count += __popcll(m);
        }
        if (tid == 0) s_count = count;
    }
    __syncthreads();
    const int cnt = s_count;
    const int CT = H >> 2, G = nthr / CT;                          // column threads, row groups
    const int g = tid / CT, c = tid - g * CT;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    if (g < G) {
#pragma unroll 4
        for (int k = g; k < cnt; k += G) {
            const size_t r = (size_t)list[k];
            if (src_bf16) {
                const bf16x4 x = *(const bf16x4*)((const bf16_t*)src + r * lds + 4 * c);
#pragma unroll
                for (int q = 0; q < 4; ++q) a[q] += bf2f(x[q]);
            } else {
                const float4 x = *(const float4*)((const float*)src + r * lds + 4 * c);
                a[0] += x.x; a[1] += x.y; a[2] += x.z; a[3] += x.w;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) red[(g * CT + c) * 4 + q] = a[q];
    }
    __syncthreads();
    if (g == 0) {
        float4* d = (float4*)(dst + (size_t)dr * ldd + 4 * c);
        float4 o = *d;
        float t[4] = {0.f, 0.f, 0.f, 0.f};
        for (int gg = 0; gg < G; ++gg)
#pragma unroll
            for (int q = 0; q < 4; ++q) t[q] += red[(gg * CT + c) * 4 + q];
        o.x += t[0]; o.y += t[1]; o.z += t[2]; o.w += t[3];
        *d = o;
    }
}

// token-type rows of the embedding scatter, deterministic mode: gtype[t][col] += sum over the positions p (ascending) of the per-position
// partial sums the scatter kernel left in slab[p][t][col]
__global__ void embed_type_fold_kernel(const float* __restrict__ slab, int T, int H, float* __restrict__ gtype) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 2 * H) return;
    float t = 0.f;
    for (int p = 0; p < T; ++p) t += slab[(size_t)p * 2 * H + e];
    gtype[e] += t;
}

#define CE_MAXC 16
// One workgroup per row, the row held in registers (<= 16 x 16 B per lane).
//   MODE 0 (forward): row_lse[i] = logsumexp(row); loss_sum[seg] += (lse - logit[label]) * inv_count[seg]
//   MODE 1 (backward): dlogits = (exp(logit - row_lse) - onehot) * inv_count[seg] * gscale[seg]
//                      (0 for ignored rows and for the pad columns V..ldv); gscale = upstream d(loss)/d(loss_seg)
// Ignored rows (label -100) are never read.
// F32: the logits are fp32 (the vocabulary GEMM's EPI_OUT_F32 output, handed to the caller as the reference's fp32 prediction scores);
// they are rounded to bf16 as they are loaded, so losses and gradients are bit-identical to the bf16-logits path.
//
// SMOOTH (label smoothing eps in (0, 1), torch's cross_entropy(label_smoothing=eps); one_minus = 1 - eps, eps_over_v = eps / V, both formed
// on the host): a compile-time form, so that the eps = 0 instantiations are the code they were.
//   forward:  loss term = lse - (1 - eps) logit[label] - (eps / V) sum_{c < V} logit[c]; the row sum of the bf16-rounded logits is taken as
//             the exp sum is (per lane in ascending (c, r), wave_sum, the four waves in order); row_lse keeps its meaning
//   backward: dlogits = (exp(logit - row_lse) - (1 - eps) onehot - eps / V) * inv_count[seg] * gscale[seg] on the columns c < V
template <int MODE, bool F32, bool SMOOTH = false>
__global__ __launch_bounds__(256) void ce_row_kernel(const void* __restrict__ logits_, int ldv, int V, const int64_t* __restrict__ labels,
                                                     const int* __restrict__ seg_bounds, int nseg, const float* __restrict__ inv_count,
                                                     float* __restrict__ loss_sum, float* __restrict__ row_lse, const float* __restrict__ gscale,
                                                     bf16_t* __restrict__ dlogits, int ldd, const int* __restrict__ rows, float* __restrict__ row_loss,
                                                     float one_minus, float eps_over_v) {
    __shared__ float red[4];
    __shared__ float lab_logit;
    const int i = rows ? rows[blockIdx.x] : blockIdx.x;        // backward over a compact row list: output row = blockIdx.x
    const int64_t lab = labels[i];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nchunk = ldv >> 3;
    if (lab < 0 || lab >= V) {
        if (MODE == 0) { if (tid == 0) { row_lse[i] = 0.f; if (row_loss) row_loss[i] = 0.f; } }
        else {
            bf16_t* drow = dlogits + (size_t)(rows ? blockIdx.x : i) * ldd;
            const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int c = tid; c < nchunk; c += 256) *(bf16x8*)(drow + c * 8) = z;
        }
        return;
    }
    int s = 0;
    while (s + 1 < nseg && i >= seg_bounds[s + 1]) ++s;
    bf16x8 v[CE_MAXC];
    if constexpr (F32) {
        const float* row = (const float*)logits_ + (size_t)i * ldv;
#pragma unroll
        for (int c = 0; c < CE_MAXC; ++c) {
            const int ch = c * 256 + tid;
            if (ch < nchunk) {
                const float4 lo = *(const float4*)(row + ch * 8), hi = *(const float4*)(row + ch * 8 + 4);
                v[c] = (bf16x8){f2bf(lo.x), f2bf(lo.y), f2bf(lo.z), f2bf(lo.w), f2bf(hi.x), f2bf(hi.y), f2bf(hi.z), f2bf(hi.w)};
            }
        }
    } else {
        const bf16_t* row = (const bf16_t*)logits_ + (size_t)i * ldv;
#pragma unroll
        for (int c = 0; c < CE_MAXC; ++c) {
            const int ch = c * 256 + tid;
            if (ch < nchunk) v[c] = *(const bf16x8*)(row + ch * 8);
        }
    }
    if (MODE == 0) {
        float mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < CE_MAXC; ++c) {
            const int ch = c * 256 + tid;
            if (ch < nchunk) {
#pragma unroll
                for (int r = 0; r < 8; ++r) if (ch * 8 + r < V) mx = fmaxf(mx, bf2f(v[c][r]));
            }
        }
        mx = wave_max(mx);
        if (lane == 0) red[w] = mx;
        __syncthreads();
        mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        __syncthreads();
        float se = 0.f;
        float sx = 0.f;                                        // SMOOTH: the row sum of the logits over the V valid columns, never a pad column
#pragma unroll
        for (int c = 0; c < CE_MAXC; ++c) {
            const int ch = c * 256 + tid;
            if (ch < nchunk) {
#pragma unroll
                for (int r = 0; r < 8; ++r) if (ch * 8 + r < V) {
                    se += __expf(bf2f(v[c][r]) - mx);
                    if constexpr (SMOOTH) sx += bf2f(v[c][r]); // (beside the exp sum: the element is converted once)
                }
                if ((int)(lab >> 3) == ch) lab_logit = bf2f(v[c][lab & 7]);
            }
        }
        se = wave_sum(se);
        if (lane == 0) red[w] = se;
        if constexpr (SMOOTH) {
            __shared__ float red_x[4];
            sx = wave_sum(sx);
            if (lane == 0) red_x[w] = sx;
            __syncthreads();
            if (tid == 0) {
                const float lse = mx + __logf(red[0] + red[1] + red[2] + red[3]);
                const float sum_x = ((red_x[0] + red_x[1]) + red_x[2]) + red_x[3];
                row_lse[i] = lse;
                const float term = __fmaf_rn(-eps_over_v, sum_x, __fmaf_rn(-one_minus, lab_logit, lse)) * inv_count[s];
                if (row_loss) row_loss[i] = term;
                else atomicAdd(loss_sum + s, term);
            }
            return;
        }
        __syncthreads();
        if (tid == 0) {
            const float lse = mx + __logf(red[0] + red[1] + red[2] + red[3]);
            row_lse[i] = lse;
            if (row_loss) row_loss[i] = (lse - lab_logit) * inv_count[s];                 // deterministic mode: summed in order by ce_loss_sum_ordered_kernel
            else atomicAdd(loss_sum + s, (lse - lab_logit) * inv_count[s]);
        }
    } else {
        const float lse = row_lse[i];
        const float scale = inv_count[s] * gscale[s];
        bf16_t* drow = dlogits + (size_t)(rows ? blockIdx.x : i) * ldd;
#pragma unroll
        for (int c = 0; c < CE_MAXC; ++c) {
            const int ch = c * 256 + tid;
            if (ch < nchunk) {
                bf16x8 o;
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const int col = ch * 8 + r;
                    float pr = col < V ? __expf(bf2f(v[c][r]) - lse) : 0.f;
                    if constexpr (SMOOTH) {
                        if (col == (int)lab) pr -= one_minus;
                        if (col < V) pr -= eps_over_v;         // (a pad column stays exactly 0)
                    } else {
                        if (col == (int)lab) pr -= 1.0f;
                    }
                    o[r] = f2bf(pr * scale);
                }
                *(bf16x8*)(drow + ch * 8) = o;
            }
        }
    }
}

// --------------------------------------------------------------------------------------------
// Vocabulary top-k (mmbert_vocab_topk): the k first columns of a logits row in the TOTAL order "larger value first, on equal values
// the lower column first", their log-probabilities, the row's logsumexp and, with a label, its log-probability and its rank in that
// order.  One workgroup per row, the row in registers as in ce_row_kernel; one pass over memory.
//
// The order as ONE unsigned compare: an element is the 32-bit word  key(value) << 16 | (0xFFFF - column)  with key() the usual
// monotone map of the bf16 bits (positive: sign bit set; negative: value bits inverted; -0 is read as +0, which it equals).  A larger
// word comes EARLIER, and no two columns share a word.  Pad columns (and register chunks past the row) carry the bits 0xFFFF, whose
// key is 0: below every real value (-inf has key 0x007F), so they are never chosen and never counted -- the scans need no bounds test.
// Round j takes the workgroup-wide largest word strictly below round j - 1's winner: no "taken" mask.  Every lane keeps its own best
// candidate; after a round only the winner's lane has lost its candidate, so only that lane scans its 128 values again (every lane
// scans once, for round 0 and the label's rank).  Lanes merge by xor shuffles, the four waves through LDS; no atomics.
// The logsumexp is ce_row_kernel<0>'s arithmetic statement for statement (max, per-lane __expf sum over c then r, wave_sum, the four
// waves in order): on a labelled row row_lse has the bits mmbert_ce_fwd writes.
// --------------------------------------------------------------------------------------------
typedef uint32_t vt_u32x4 __attribute__((ext_vector_type(4)));

// bf16 bits in the HIGH half of h (low half zero) -> sortable key in the high half, low half zero
__device__ __forceinline__ uint32_t vt_key(uint32_t h) {
    const uint32_t neg = (uint32_t)((int32_t)h >> 31);
    return h ^ ((neg & 0x7FFF0000u) | 0x80000000u);
}
__device__ __forceinline__ float vt_value(uint32_t word) {      // the value behind an order word
    const uint32_t kk = word & 0xFFFF0000u;
    return __builtin_bit_cast(float, (kk & 0x80000000u) ? (kk ^ 0x80000000u) : (kk ^ 0xFFFF0000u));
}
__device__ __forceinline__ uint32_t vt_wave_max(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
    return v;
}
// a lane's largest order word strictly below `prev` (0: none); COUNT: also how many of its words lie above `lab_word`.
// e - prev in unsigned arithmetic puts every word below prev above every word at or past it, the closest one highest: one subtraction
// and one max per element.
template <bool COUNT>
__device__ __forceinline__ uint32_t vt_scan(const uint32_t (&e)[CE_MAXC * 8], uint32_t prev, uint32_t lab_word, int& above) {
    uint32_t best = 0u;
#pragma unroll
    for (int n = 0; n < CE_MAXC * 8; ++n) {
        best = max(best, e[n] - prev);
        if (COUNT) above += e[n] > lab_word ? 1 : 0;
    }
    const uint32_t word = best + prev;
    return word < prev ? word : 0u;
}

template <bool F32>
__global__ __launch_bounds__(256) void vocab_topk_kernel(const void* __restrict__ logits_, int ldv, int V, int k, const int64_t* __restrict__ labels,
                                                         int32_t* __restrict__ top_ids, float* __restrict__ top_logprob, float* __restrict__ row_lse,
                                                         float* __restrict__ label_logprob, int32_t* __restrict__ label_rank) {
    __shared__ float red[4];
    __shared__ float lab_logit;
    __shared__ int red_above[4];
    __shared__ uint32_t red_word[2][4];
    const int i = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nchunk = (V + 7) >> 3;                           // <= CE_MAXC * 256; pad columns past the last of these are never loaded
    const int64_t lab = labels ? labels[i] : -1;
    const bool has_lab = lab >= 0 && lab < V;                  // workgroup-uniform
    const int lab_chunk = has_lab ? (int)(lab >> 3) : -1;
    bf16x8 v[CE_MAXC];
    if constexpr (F32) {
        const float* row = (const float*)logits_ + (size_t)i * ldv;
#pragma unroll
        for (int c = 0; c < CE_MAXC; ++c) {
            const int ch = c * 256 + tid;
            if (ch < nchunk) {
                const float4 lo = *(const float4*)(row + ch * 8), hi = *(const float4*)(row + ch * 8 + 4);
                v[c] = (bf16x8){f2bf(lo.x), f2bf(lo.y), f2bf(lo.z), f2bf(lo.w), f2bf(hi.x), f2bf(hi.y), f2bf(hi.z), f2bf(hi.w)};
            }
        }
    } else {
        const bf16_t* row = (const bf16_t*)logits_ + (size_t)i * ldv;
#pragma unroll
        for (int c = 0; c < CE_MAXC; ++c) {
            const int ch = c * 256 + tid;
            if (ch < nchunk) v[c] = *(const bf16x8*)(row + ch * 8);
        }
    }
    // ---- logsumexp: ce_row_kernel<0>
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < CE_MAXC; ++c) {
        const int ch = c * 256 + tid;
        if (ch < nchunk) {
#pragma unroll
            for (int r = 0; r < 8; ++r) if (ch * 8 + r < V) mx = fmaxf(mx, bf2f(v[c][r]));
        }
    }
    mx = wave_max(mx);
    if (lane == 0) red[w] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float se = 0.f;
    {
        // the per-lane sum in ascending (c, r) order, as ce_row_kernel's is emitted: pinned, so that -ffast-math cannot re-associate it here
#pragma clang fp reassociate(off)
#pragma unroll
        for (int c = 0; c < CE_MAXC; ++c) {
            const int ch = c * 256 + tid;
            if (ch < nchunk) {
#pragma unroll
                for (int r = 0; r < 8; ++r) if (ch * 8 + r < V) se += __expf(bf2f(v[c][r]) - mx);
            }
        }
    }
    if (lab_chunk >= 0) {                                       // (outside the sum's loop: nothing but the sum in the pinned block)
#pragma unroll
        for (int c = 0; c < CE_MAXC; ++c)
            if (lab_chunk == c * 256 + tid) lab_logit = bf2f(v[c][lab & 7]);
    }
    se = wave_sum(se);
    if (lane == 0) red[w] = se;
    __syncthreads();
    float lse = 0.f;
    if (tid == 0) {
        float tot;
        {
            // the four waves in ce_row_kernel's order: the library is built with -ffast-math, and left free the compiler pairs them here
            // ((0 + 2) + (1 + 3) through one packed add), which moves the last bit of the lse on some rows
#pragma clang fp reassociate(off)
            tot = ((red[0] + red[1]) + red[2]) + red[3];
        }
        lse = mx + __logf(tot);
        row_lse[i] = lse;
    }
    // ---- the row as order words: -0 -> +0, pad columns and absent chunks -> key 0
    uint32_t e[CE_MAXC * 8];
#pragma unroll
    for (int c = 0; c < CE_MAXC; ++c) {
        const int ch = c * 256 + tid;
        const vt_u32x4 t = __builtin_bit_cast(vt_u32x4, v[c]);
        const uint32_t low = 0xFFFFu - (uint32_t)(ch * 8);     // 0xFFFF - column of the chunk's first element (ch * 8 + 7 <= 32767 where ch < nchunk)
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            uint32_t h0 = t[d] << 16, h1 = t[d] & 0xFFFF0000u;
            const int col = ch * 8 + 2 * d;
            if (h0 == 0x80000000u) h0 = 0u;
            if (h1 == 0x80000000u) h1 = 0u;
            if (ch >= nchunk || col >= V) h0 = 0xFFFF0000u;
            if (ch >= nchunk || col + 1 >= V) h1 = 0xFFFF0000u;
            e[c * 8 + 2 * d] = vt_key(h0) | ((low - (uint32_t)(2 * d)) & 0xFFFFu);
            e[c * 8 + 2 * d + 1] = vt_key(h1) | ((low - (uint32_t)(2 * d + 1)) & 0xFFFFu);
        }
    }
    // ---- every lane's first candidate, and the label's rank = the number of words above the label's own
    uint32_t lab_word = 0u;
    float lab_x = 0.f;
    int above = 0;
    uint32_t mine;
    if (has_lab) {
        lab_x = lab_logit;                                     // (written before the barrier above)
        uint32_t hb = __builtin_bit_cast(uint32_t, lab_x);
        if (hb == 0x80000000u) hb = 0u;
        lab_word = vt_key(hb) | (0xFFFFu - (uint32_t)lab);
        mine = vt_scan<true>(e, 0xFFFFFFFFu, lab_word, above);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) above += __shfl_xor(above, o, 64);
        if (lane == 0) red_above[w] = above;
    } else {
        mine = vt_scan<false>(e, 0xFFFFFFFFu, 0u, above);
    }
    // ---- k rounds
    for (int j = 0; j < k; ++j) {
        const uint32_t wm = vt_wave_max(mine);
        if (lane == 0) red_word[j & 1][w] = wm;
        __syncthreads();                                       // (round j + 2 rewrites this slot behind round j + 1's barrier)
        const uint32_t win = max(max(red_word[j & 1][0], red_word[j & 1][1]), max(red_word[j & 1][2], red_word[j & 1][3]));
        if (tid == 0) {
            top_ids[(size_t)i * k + j] = (int32_t)(0xFFFFu - (win & 0xFFFFu));
            top_logprob[(size_t)i * k + j] = vt_value(win) - lse;
        }
        if (j + 1 < k && mine == win) mine = vt_scan<false>(e, win, 0u, above);
    }
    if (tid == 0 && label_logprob) {
        if (has_lab) {
            label_logprob[i] = lab_x - lse;
            label_rank[i] = red_above[0] + red_above[1] + red_above[2] + red_above[3];
        } else {
            label_logprob[i] = 0.f;
            label_rank[i] = -1;
        }
    }
}

// --------------------------------------------------------------------------------------------
// Flat AdamW over the model's contiguous fp32 parameter / gradient / moment buffers.
// flags[block of 256 elements]: 0 = no weight decay, 1 = weight decay, 2 = frozen (the
// reference's never-differentiated parameters keep grad None and are skipped by the optimizer);
// + 4 = "the next backward OVERWRITES this block's gradient" (flat.FlatParams lazy zero: the fused zero_grad
// leaves the block alone -- torch's zero_grad(set_to_none=True) does not touch the old gradient either).
// mode 0 = transformers-2.8 AdamW (decay after the update), 1 = torch.optim.AdamW.
// Also writes the bf16 working copy and (optionally) zeroes the gradient: zero_grad fused.
// --------------------------------------------------------------------------------------------
// The eight scalar coefficients of one hyper-parameter set, ready-made (adamw_coefs forms them in double and rounds once): omb1 / omb2 =
// 1 - beta1 / 1 - beta2; step_size = lr sqrt(bc2) / bc1 (mode 0) or lr / bc1 (mode 1); rsbc2 = 1 / sqrt(bc2) (mode 1); lrwd = lr * wd.
struct AdamWCoefs { float beta1, beta2, omb1, omb2, eps, step_size, rsbc2, lrwd; };

// One element of the update, with the rounding fixed in the source.  The library is built with -ffast-math: which multiply of
// beta1 m + omb1 gr is fused into the FMA, and how the division and the square root are expanded, is then the compiler's choice, and it
// made another one when the plain expressions of the four kernels were moved into one shared body: every stored bit of a training
// trajectory moved.  So each FMA is named with its operand roles, the square root and the reciprocal are the hardware approximations
// (v_sqrt_f32, v_rcp_f32) by name, and contraction and reassociation are off here: every kernel below computes this dataflow and no other.
__device__ __forceinline__ void adamw_element(float& p, float g, float& m, float& v, const AdamWCoefs& c, float decay, float gscale, int mode) {
#pragma clang fp contract(off)
#pragma clang fp reassociate(off)
    const float gr = g * gscale;
    if (mode == 1) p = p * (1.0f - decay);
    m = __builtin_fmaf(c.omb1, gr, c.beta1 * m);
    v = __builtin_fmaf(c.omb2, gr * gr, c.beta2 * v);
    const float rt = __builtin_amdgcn_sqrtf(v), upd = c.step_size * m;
    if (mode == 0) {
        p = __builtin_fmaf(-upd, __builtin_amdgcn_rcpf(rt + c.eps), p);
        p = __builtin_fmaf(-p, decay, p);
    } else {
        p = __builtin_fmaf(-upd, __builtin_amdgcn_rcpf(__builtin_fmaf(c.rsbc2, rt, c.eps)), p);
    }
}

// ema += omd (p - ema), one element: a subtract, then one FMA onto e (the form e + omd (p - e) keeps updates that are small against e
// at decay 0.9999).  Pinned like adamw_element.
__device__ __forceinline__ float ema_element(float e, float p, float omd) {
#pragma clang fp contract(off)
#pragma clang fp reassociate(off)
    return __builtin_fmaf(p - e, omd, e);
}

// The lane's first element (four per lane, 256 lanes per workgroup); n % 256 == 0, so a lane is wholly inside or wholly outside.
__device__ __forceinline__ size_t adamw_lane_element() { return ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; }

// The body of every AdamW kernel, for the lane whose elements start at i < n: the flag byte, the live / frozen split, the update of
// p, m, v (and of ema, when EMA), the fused zero_grad, the bf16 refresh.  coefs() yields the block's AdamWCoefs and is called for live
// blocks only: the kernels differ in where it reads them, in where gscale comes from and in EMA, and in nothing else.
template <bool EMA, class Coefs>
__device__ __forceinline__ void adamw_update(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                             float* __restrict__ ema, bf16_t* __restrict__ pb, const uint8_t* __restrict__ flags, size_t i,
                                             Coefs coefs, float gscale, float omd, int mode, int zero_grad) {
    const uint8_t fb = flags[i >> 8];
    const uint8_t f = fb & 3;
    float4 P = *(float4*)(p + i);
    if (f != 2) {
        const AdamWCoefs c = coefs();
        float4 G = *(float4*)(g + i), Mm = *(float4*)(m + i), Vv = *(float4*)(v + i), E;
        if (EMA) E = *(float4*)(ema + i);
        float pa[4] = {P.x, P.y, P.z, P.w}, ga[4] = {G.x, G.y, G.z, G.w}, ma[4] = {Mm.x, Mm.y, Mm.z, Mm.w}, va[4] = {Vv.x, Vv.y, Vv.z, Vv.w};
        const float decay = (f == 1) ? c.lrwd : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) adamw_element(pa[r], ga[r], ma[r], va[r], c, decay, gscale, mode);
        P = make_float4(pa[0], pa[1], pa[2], pa[3]);
        *(float4*)(p + i) = P;
        *(float4*)(m + i) = make_float4(ma[0], ma[1], ma[2], ma[3]);
        *(float4*)(v + i) = make_float4(va[0], va[1], va[2], va[3]);
        if (EMA)
            *(float4*)(ema + i) = make_float4(ema_element(E.x, P.x, omd), ema_element(E.y, P.y, omd), ema_element(E.z, P.z, omd),
                                              ema_element(E.w, P.w, omd));
    }
    if (zero_grad && !(fb & 4)) *(float4*)(g + i) = make_float4(0.f, 0.f, 0.f, 0.f);
    if (pb) { bf16x4 o = {f2bf(P.x), f2bf(P.y), f2bf(P.z), f2bf(P.w)}; *(bf16x4*)(pb + i) = o; }
}

// One hyper-parameter set, its coefficients in the kernel's scalar arguments; the gradient scale from the host.
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                    bf16_t* __restrict__ pb, const uint8_t* __restrict__ flags, size_t n,
                                                    float beta1, float beta2, float omb1, float omb2, float eps, float step_size, float rsbc2, float lrwd,
                                                    float gscale, int mode, int zero_grad) {
    const size_t i = adamw_lane_element();
    if (i >= n) return;
    adamw_update<false>(p, g, m, v, nullptr, pb, flags, i, [&] { return AdamWCoefs{beta1, beta2, omb1, omb2, eps, step_size, rsbc2, lrwd}; },
                        gscale, 0.f, mode, zero_grad);
}

// adamw_kernel with the gradient scale read from the DEVICE scalar *coef (the clip coefficient of mmbert_grad_norm with the 1/world
// average folded in; one scalar load per wave) in place of the host gscale.  A kernel of its own, like the two below, for its name in
// the traces and so that adamw_kernel's arguments stay as they are; the arithmetic is adamw_update's in all of them.
__global__ __launch_bounds__(256) void adamw_devscale_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                             bf16_t* __restrict__ pb, const uint8_t* __restrict__ flags, size_t n,
                                                             float beta1, float beta2, float omb1, float omb2, float eps, float step_size, float rsbc2,
                                                             float lrwd, const float* __restrict__ coef, int mode, int zero_grad) {
    const size_t i = adamw_lane_element();
    if (i >= n) return;
    adamw_update<false>(p, g, m, v, nullptr, pb, flags, i, [&] { return AdamWCoefs{beta1, beta2, omb1, omb2, eps, step_size, rsbc2, lrwd}; },
                        *coef, 0.f, mode, zero_grad);
}

// Per-parameter-group AdamW (torch / transformers param groups with their own lr, betas, eps, weight_decay).  group_of_block[i / 256]
// names each 256-element block's group, at the granularity of flags; slot[group] picks one of the de-duplicated coefficient sets that
// adamw_fill_slots formed in double and rounded to fp32 once.  The whole table travels BY VALUE in the kernel arguments: no device
// allocation, no copy per step (the host runs a step ahead), nothing to sync, graph-capturable.  One wave = 64 lanes x 4 floats = one
// block, so the group is wave-uniform: readfirstlane makes that provable and the slot word and the 8 coefficients come in as scalar
// loads from the argument segment, once per wave.  The update is adamw_kernel's (same traffic + 1 byte per block).
#define ADAMW_MAX_GROUPS 255             // == MMBERT_ADAMW_MAX_GROUPS (include/mmbert_hip.h)
#define ADAMW_MAX_SLOTS 64               // == MMBERT_ADAMW_MAX_SLOTS
struct AdamWSlots {
    AdamWCoefs c[ADAMW_MAX_SLOTS];
    uint32_t slot4[64];                  // group k -> slot in byte k & 3 of word k >> 2 (a word: one scalar load; 256 entries = every
                                         // value of a group byte, so a stray index reads slot 0, never past the table)
};
static_assert(sizeof(AdamWSlots) == 2304, "AdamWSlots layout");
static_assert(sizeof(AdamWSlots) + 128 <= 4096, "adamw_grouped_kernel's arguments must fit the 4 KiB kernel-argument segment");

__device__ __forceinline__ AdamWCoefs adamw_slot_coefs(const AdamWSlots& a, int grp) {
    return a.c[(a.slot4[grp >> 2] >> ((grp & 3) * 8)) & 255u];
}

template <bool DEVSCALE>
__global__ __launch_bounds__(256) void adamw_grouped_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                            bf16_t* __restrict__ pb, const uint8_t* __restrict__ flags,
                                                            const uint8_t* __restrict__ group_of_block, size_t n, const AdamWSlots a,
                                                            float host_gscale, const float* __restrict__ coef, int mode, int zero_grad) {
    const size_t i = adamw_lane_element();
    if (i >= n) return;
    const float gscale = DEVSCALE ? *coef : host_gscale;
    const int grp = __builtin_amdgcn_readfirstlane((int)group_of_block[i >> 8]);
    adamw_update<false>(p, g, m, v, nullptr, pb, flags, i, [&] { return adamw_slot_coefs(a, grp); }, gscale, 0.f, mode, zero_grad);
}

// adamw_grouped_kernel plus an exponential moving average of the weights: once a live block's new p is formed (it is in registers),
// ema += omd * (p - ema) with omd = 1 - decay (mmbert_adamw_ema forms it in double and rounds once).  Frozen blocks (flag 2) leave ema
// alone.  group_of_block == NULL: every block is group 0 (one hyper-parameter set: the table then holds mmbert_adamw's coefficients in
// slot 0).  The update of p, m, v, g and the bf16 copy is adamw_update's, the one body of all four kernels, so turning the average on
// moves no bit of a training trajectory -- by construction.  New traffic: one float4 load and one store of ema per lane (36 B/parameter).
template <bool DEVSCALE>
__global__ __launch_bounds__(256) void adamw_ema_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                        float* __restrict__ ema, bf16_t* __restrict__ pb, const uint8_t* __restrict__ flags,
                                                        const uint8_t* __restrict__ group_of_block, size_t n, const AdamWSlots a,
                                                        float host_gscale, const float* __restrict__ coef, float omd, int mode, int zero_grad) {
    const size_t i = adamw_lane_element();
    if (i >= n) return;
    const float gscale = DEVSCALE ? *coef : host_gscale;
    const int grp = group_of_block ? __builtin_amdgcn_readfirstlane((int)group_of_block[i >> 8]) : 0;
    adamw_update<true>(p, g, m, v, ema, pb, flags, i, [&] { return adamw_slot_coefs(a, grp); }, gscale, omd, mode, zero_grad);
}

// p <-> ema, and the bf16 working copy of the new p (mmbert_cast_f32_bf16's rounding), in one pass: 16 B/parameter + 2 for the copy, no
// temporary.  Indexed like the AdamW kernels (n % 256 == 0: whole float4s).
__global__ __launch_bounds__(256) void ema_swap_kernel(float* __restrict__ p, float* __restrict__ ema, bf16_t* __restrict__ pb, size_t n) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    const float4 P = *(float4*)(p + i), E = *(float4*)(ema + i);
    *(float4*)(p + i) = E;
    *(float4*)(ema + i) = P;
    if (pb) { bf16x4 o = {f2bf(E.x), f2bf(E.y), f2bf(E.z), f2bf(E.w)}; *(bf16x4*)(pb + i) = o; }
}

// --------------------------------------------------------------------------------------------
// Flat LAMB (You et al., Algorithm 2 with bias correction; apex FusedLAMB's defaults) over the buffers, flags and groups of the AdamW
// kernels: the Adam moments, then per parameter tensor (a TRUST UNIT) r = ||p|| / ||u|| of u = mhat / (sqrt(vhat) + eps) + wd p, then
// p -= lr r u.  Three launches, no atomics, nothing read back:
//   1. lamb_moments_kernel  p, g, m, v -> m, v; sum p^2 and sum u^2 of every wave's block into its slot(s) of the partials slab
//   2. lamb_fold_kernel     one workgroup per unit: its slots in a fixed order, in double -> (r, ||p||, ||u||)
//   3. lamb_apply_kernel    p, m, v -> u again through lamb_u (the bits that were measured are the bits applied), p, bf16, zero_grad, ema
// Units follow the tensors, not the blocks (flat.FlatParams packs a LayerNorm's weight and bias or the q / k / v biases into one block):
// unit_of_block[b] >= 0 is the unit of a PURE block (slot b of the slab); -(k + 1) names record k of `mixed`, eight ints
// (q0, u0, q1, u1, q2, u2, q3, u3): lanes q_e <= lane < q_(e+1) of the wave (a lane holds one aligned float4: a quad) belong to unit
// u_e; q0 = 0, ascending, an unused entry has q = 64; u_e = -1 is "no unit" (ratio 1, nothing measured).  Entry e of record k owns
// slot nblk + 4 k + e.  Stray indices are clamped into their tables: nothing is read or written past them.
// --------------------------------------------------------------------------------------------
struct LambCoefs { float beta1, beta2, omb1, omb2, eps, rbc1, rbc2, lr, wd; };   // rbc = 1 / (1 - beta^step), in double, rounded once
struct LambSlots {
    LambCoefs c[ADAMW_MAX_SLOTS];
    uint32_t slot4[64];                  // as AdamWSlots::slot4
};
static_assert(sizeof(LambSlots) + 160 <= 4096, "the LAMB kernels' arguments must fit the 4 KiB kernel-argument segment");

__device__ __forceinline__ LambCoefs lamb_slot_coefs(const LambSlots& a, int grp) {
    return a.c[(a.slot4[grp >> 2] >> ((grp & 3) * 8)) & 255u];
}

// adamw_element's two moment lines, FMA for FMA under the same pragmas: m and v get the bits mmbert_adamw_grouped writes.
__device__ __forceinline__ void lamb_moments_element(float g, float& m, float& v, const LambCoefs& c, float gscale) {
#pragma clang fp contract(off)
#pragma clang fp reassociate(off)
    const float gr = g * gscale;
    m = __builtin_fmaf(c.omb1, gr, c.beta1 * m);
    v = __builtin_fmaf(c.omb2, gr * gr, c.beta2 * v);
}

// u of one element, pinned like adamw_element (v_sqrt_f32, v_rcp_f32 by name): launches 1 and 3 both call this on the same p, m, v.
__device__ __forceinline__ float lamb_u(float p, float m, float v, const LambCoefs& c, float wd) {
#pragma clang fp contract(off)
#pragma clang fp reassociate(off)
    const float den = __builtin_amdgcn_sqrtf(v * c.rbc2) + c.eps;
    return __builtin_fmaf(wd, p, (m * c.rbc1) * __builtin_amdgcn_rcpf(den));
}

__device__ __forceinline__ float lamb_wave_sum(float a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);          // xor butterfly: a fixed order, the same sum in every lane
    return a;
}

// The mixed-block record of map entry e < 0, clamped into the table.
__device__ __forceinline__ const int* lamb_record(const int* __restrict__ mixed, int nmixed, int e, int& k) {
    k = min(max(-e - 1, 0), nmixed - 1);
    return mixed + 8 * (size_t)k;
}

template <bool DEVSCALE>
__global__ __launch_bounds__(256) void lamb_moments_kernel(const float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, const uint8_t* __restrict__ flags,
                                                           const uint8_t* __restrict__ group_of_block, const int* __restrict__ unit_of_block,
                                                           const int* __restrict__ mixed, int nmixed, size_t n, const LambSlots a,
                                                           float host_gscale, const float* __restrict__ coef, float2* __restrict__ part) {
    const size_t i = adamw_lane_element();
    if (i >= n) return;
    const size_t b = i >> 8, nblk = n >> 8;
    const uint8_t f = flags[b] & 3;
    if (f == 2) return;                                                   // frozen: in no unit, nothing stored
    const float gscale = DEVSCALE ? *coef : host_gscale;
    const int grp = group_of_block ? __builtin_amdgcn_readfirstlane((int)group_of_block[b]) : 0;
    const LambCoefs c = lamb_slot_coefs(a, grp);
    const float wd = (f == 1) ? c.wd : 0.f;
    const float4 P = *(const float4*)(p + i), G = *(const float4*)(g + i), Mm = *(float4*)(m + i), Vv = *(float4*)(v + i);
    const float pa[4] = {P.x, P.y, P.z, P.w}, ga[4] = {G.x, G.y, G.z, G.w};
    float ma[4] = {Mm.x, Mm.y, Mm.z, Mm.w}, va[4] = {Vv.x, Vv.y, Vv.z, Vv.w};
    float sp = 0.f, su = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        lamb_moments_element(ga[r], ma[r], va[r], c, gscale);
        const float u = lamb_u(pa[r], ma[r], va[r], c, wd);
        sp = fmaf(pa[r], pa[r], sp);
        su = fmaf(u, u, su);
    }
    *(float4*)(m + i) = make_float4(ma[0], ma[1], ma[2], ma[3]);
    *(float4*)(v + i) = make_float4(va[0], va[1], va[2], va[3]);
    const int lane = threadIdx.x & 63;
    const int e = __builtin_amdgcn_readfirstlane(unit_of_block[b]);
    if (e >= 0) {
        const float tp = lamb_wave_sum(sp), tu = lamb_wave_sum(su);
        if (lane == 0) part[b] = make_float2(tp, tu);
    } else if (nmixed > 0) {
        int k;
        const int* rec = lamb_record(mixed, nmixed, e, k);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int q0 = rec[2 * s], q1 = s < 3 ? rec[2 * s + 2] : 64, unit = rec[2 * s + 1];
            if (q0 >= 64 || unit < 0) continue;                           // (wave-uniform: the record is read with scalar loads)
            const bool mine = lane >= q0 && lane < q1;
            const float tp = lamb_wave_sum(mine ? sp : 0.f), tu = lamb_wave_sum(mine ? su : 0.f);
            if (lane == 0) part[nblk + 4 * (size_t)k + s] = make_float2(tp, tu);
        }
    }
}

// units[4 T ..] = (first block, one past the last block, adapt, 0) of unit T: the blocks that can hold a part of it.  ratios[3 T ..] =
// (r, ||p||, ||u||): r = ||p|| / ||u|| when adapt != 0 and both are > 0, else 1; then min(r, max_trust) when max_trust > 0.  Every thread
// adds its blocks' slots in ascending order, the threads are then added in a fixed tree: the bits depend on the data alone.
#define LAMB_FOLD_THREADS 1024
#define LAMB_FOLD_UNROLL 8
__global__ __launch_bounds__(LAMB_FOLD_THREADS) void lamb_fold_kernel(const float2* __restrict__ part, const uint8_t* __restrict__ flags,
                                                                      const int* __restrict__ unit_of_block, const int* __restrict__ mixed,
                                                                      int nmixed, const int* __restrict__ units, int nblk, float max_trust,
                                                                      float* __restrict__ ratios) {
    __shared__ double red[2][LAMB_FOLD_THREADS / 64];
    const int T = blockIdx.x;
    const int b0 = min(max(units[4 * T], 0), nblk), b1 = min(max(units[4 * T + 1], b0), nblk), adapt = units[4 * T + 2];
    double sp = 0.0, su = 0.0;
    for (int base = b0 + (int)threadIdx.x; base < b1; base += LAMB_FOLD_UNROLL * LAMB_FOLD_THREADS) {
        int e[LAMB_FOLD_UNROLL];
        uint8_t fl[LAMB_FOLD_UNROLL];
        float2 x[LAMB_FOLD_UNROLL];
#pragma unroll
        for (int u = 0; u < LAMB_FOLD_UNROLL; ++u) {                      // issued together (the word table's unit has 90k blocks); the
            const int b = min(base + u * LAMB_FOLD_THREADS, b1 - 1);      // pure slot is read before it is known to be one: b < nblk
            e[u] = unit_of_block[b]; fl[u] = flags[b]; x[u] = part[b];
        }
#pragma unroll
        for (int u = 0; u < LAMB_FOLD_UNROLL; ++u) {
            if (base + u * LAMB_FOLD_THREADS >= b1 || (fl[u] & 3) == 2) continue;
            if (e[u] >= 0) {
                if (e[u] == T) { sp += (double)x[u].x; su += (double)x[u].y; }
            } else if (nmixed > 0) {
                int k;
                const int* rec = lamb_record(mixed, nmixed, e[u], k);
                for (int s = 0; s < 4; ++s)
                    if (rec[2 * s] < 64 && rec[2 * s + 1] == T) {
                        const float2 y = part[(size_t)nblk + 4 * (size_t)k + s];
                        sp += (double)y.x; su += (double)y.y;
                    }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sp += __shfl_xor(sp, o, 64); su += __shfl_xor(su, o, 64); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sp; red[1][threadIdx.x >> 6] = su; }
    __syncthreads();
    if (threadIdx.x == 0) {
        sp = red[0][0]; su = red[1][0];
        for (int w = 1; w < LAMB_FOLD_THREADS / 64; ++w) { sp += red[0][w]; su += red[1][w]; }
        const double np = sqrt(sp), nu = sqrt(su);
        float r = (adapt && np > 0.0 && nu > 0.0) ? (float)(np / nu) : 1.f;
        if (max_trust > 0.f && r > max_trust) r = max_trust;
        ratios[3 * T] = r; ratios[3 * T + 1] = (float)np; ratios[3 * T + 2] = (float)nu;
    }
}

template <bool EMA>
__global__ __launch_bounds__(256) void lamb_apply_kernel(float* __restrict__ p, float* __restrict__ g, const float* __restrict__ m,
                                                         const float* __restrict__ v, float* __restrict__ ema, bf16_t* __restrict__ pb,
                                                         const uint8_t* __restrict__ flags, const uint8_t* __restrict__ group_of_block,
                                                         const int* __restrict__ unit_of_block, const int* __restrict__ mixed, int nmixed,
                                                         const float* __restrict__ ratios, int nunits, size_t n, const LambSlots a,
                                                         float omd, int zero_grad) {
    const size_t i = adamw_lane_element();
    if (i >= n) return;
    const size_t b = i >> 8;
    const uint8_t fb = flags[b];
    const uint8_t f = fb & 3;
    float4 P = *(float4*)(p + i);
    if (f != 2) {
        const int grp = group_of_block ? __builtin_amdgcn_readfirstlane((int)group_of_block[b]) : 0;
        const LambCoefs c = lamb_slot_coefs(a, grp);
        const float wd = (f == 1) ? c.wd : 0.f;
        const float4 Mm = *(const float4*)(m + i), Vv = *(const float4*)(v + i);
        float4 E;
        if (EMA) E = *(float4*)(ema + i);
        const int e = __builtin_amdgcn_readfirstlane(unit_of_block[b]);
        float r = 1.f;
        if (e >= 0) {
            r = ratios[3 * (size_t)min(e, nunits - 1)];                   // wave-uniform: one scalar load
        } else if (nmixed > 0) {
            int k;
            const int* rec = lamb_record(mixed, nmixed, e, k);
            const int lane = threadIdx.x & 63;
            int unit = rec[1];
#pragma unroll
            for (int s = 1; s < 4; ++s) unit = (lane >= rec[2 * s]) ? rec[2 * s + 1] : unit;
            if (unit >= 0) r = ratios[3 * (size_t)min(unit, nunits - 1)];
        }
        float pa[4] = {P.x, P.y, P.z, P.w};
        const float ma[4] = {Mm.x, Mm.y, Mm.z, Mm.w}, va[4] = {Vv.x, Vv.y, Vv.z, Vv.w};
        const float step = c.lr * r;
#pragma unroll
        for (int q = 0; q < 4; ++q) pa[q] = __builtin_fmaf(-step, lamb_u(pa[q], ma[q], va[q], c, wd), pa[q]);
        P = make_float4(pa[0], pa[1], pa[2], pa[3]);
        *(float4*)(p + i) = P;
        if (EMA)
            *(float4*)(ema + i) = make_float4(ema_element(E.x, P.x, omd), ema_element(E.y, P.y, omd), ema_element(E.z, P.z, omd),
                                              ema_element(E.w, P.w, omd));
    }
    if (zero_grad && !(fb & 4)) *(float4*)(g + i) = make_float4(0.f, 0.f, 0.f, 0.f);
    if (pb) { bf16x4 o = {f2bf(P.x), f2bf(P.y), f2bf(P.z), f2bf(P.w)}; *(bf16x4*)(pb + i) = o; }
}

// --------------------------------------------------------------------------------------------
// Global gradient norm over a list of element segments of a flat fp32 buffer (torch.nn.utils.clip_grad_norm_: the reference
// never clips; BERT's recipe and HF Trainer clip at 1.0).  segs[2 s], segs[2 s + 1] = offset, length of
// segment s in elements -- any offset, any length: parameters pack inside 256-element blocks (flat.py ALIGN).
// Every access is a 16-byte load of the aligned float4 that holds the elements; the lanes outside the segment are masked
// (a straddling float4 at a segment edge is read whole, its foreign elements select 0).  Only the buffer's own last partial float4
// (n % 4 != 0) is read element by element, clamped to n - 1.
// Two launches, no float atomics, no in-launch hand-off between workgroups (the per-XCD L2s are not coherent: DESIGN 3.5,
// tools/ubench/exchange_check.py): every
// workgroup STORES its partial (double) into its own slot; one workgroup then folds the slots in slot order.  Squares are summed in
// fp32 per lane (GN_UNROLL x 4 independent accumulators, ~30 terms each at the headline size), in double from there on.  The grid
// depends on n alone (sized for 256 CUs, not from a device query), so the bits depend on the data alone.
// --------------------------------------------------------------------------------------------
#define GN_THREADS 256
#define GN_UNROLL 4
#define GN_MAX_WG 1024                   // 256 CUs x 4; == MMBERT_GRAD_NORM_WORKSPACE / sizeof(double)

template <bool INF>
__device__ __forceinline__ double gn_combine(double a, double b) {
    if (!INF) return a + b;
    return (b > a || __builtin_isnan(b)) ? b : a;               // max that keeps a NaN (torch's amax / clamp propagate it)
}

template <bool INF>
__device__ __forceinline__ float gn_acc(float a, float x) {
    if (!INF) return fmaf(x, x, a);
    const float ax = fabsf(x);
    return (ax > a || __builtin_isnan(ax)) ? ax : a;
}

// lane -> wave (xor butterfly, fixed order) -> workgroup (4 waves, slot order); the result is valid in thread 0
template <bool INF>
__device__ __forceinline__ double gn_block_reduce(double a) {
    __shared__ double red[GN_THREADS / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a = gn_combine<INF>(a, __shfl_xor(a, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        a = red[0];
#pragma unroll
        for (int w = 1; w < GN_THREADS / 64; ++w) a = gn_combine<INF>(a, red[w]);
    }
    return a;
}

template <bool INF>
__global__ __launch_bounds__(GN_THREADS) void grad_norm_partial_kernel(const float* __restrict__ g, size_t n, const long long* __restrict__ segs,
                                                                       int nseg, double* __restrict__ part) {
    const size_t T = (size_t)gridDim.x * GN_THREADS, t = (size_t)blockIdx.x * GN_THREADS + threadIdx.x;
    const size_t nfull = n >> 2;                                 // float4s wholly inside the buffer
    float acc[GN_UNROLL][4];
#pragma unroll
    for (int u = 0; u < GN_UNROLL; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[u][r] = 0.f;
    for (int s = 0; s < nseg; ++s) {
        const size_t lo = min((size_t)segs[2 * s], n), hi = min(lo + (size_t)segs[2 * s + 1], n);
        const size_t c0 = lo >> 2, c1 = min((hi + 3) >> 2, nfull);
        for (size_t c = c0 + t; c < c1; c += GN_UNROLL * T) {
            float4 x[GN_UNROLL];
#pragma unroll
            for (int u = 0; u < GN_UNROLL; ++u) x[u] = *(const float4*)(g + 4 * min(c + u * T, c1 - 1));       // issued together
#pragma unroll
            for (int u = 0; u < GN_UNROLL; ++u) {
                const size_t e = 4 * (c + u * T);
                const bool live = c + u * T < c1;
                const float xs[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[u][r] = gn_acc<INF>(acc[u][r], (live && e + r >= lo && e + r < hi) ? xs[r] : 0.f);
            }
        }
        if (t == 0 && hi > 4 * nfull && lo < hi) {               // the buffer's last partial float4 (n % 4 != 0)
            float xs[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) xs[r] = g[min(4 * nfull + r, n - 1)];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const size_t e = 4 * nfull + r;
                acc[0][r] = gn_acc<INF>(acc[0][r], (e >= lo && e < hi) ? xs[r] : 0.f);
            }
        }
    }
    double a = 0.0;
#pragma unroll
    for (int u = 0; u < GN_UNROLL; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) a = gn_combine<INF>(a, (double)acc[u][r]);
    a = gn_block_reduce<INF>(a);
    if (threadIdx.x == 0) part[blockIdx.x] = a;
}

// out[0] = ||gscale g|| (fp32), out[1] = min(1, max_norm / (out[0] + 1e-6)) in fp32 as torch forms it (NaN stays NaN, max_norm / inf = 0),
// out[2] = out[1] * gscale (the factor the AdamW kernel applies to the raw gradient)
template <bool INF>
__global__ __launch_bounds__(GN_THREADS) void grad_norm_finalize_kernel(const double* __restrict__ part, int nparts, float max_norm, double gscale,
                                                                        float* __restrict__ out) {
    double x[GN_MAX_WG / GN_THREADS];
#pragma unroll
    for (int k = 0; k < GN_MAX_WG / GN_THREADS; ++k) x[k] = part[min((int)threadIdx.x + k * GN_THREADS, nparts - 1)];     // issued together
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < GN_MAX_WG / GN_THREADS; ++k) a = gn_combine<INF>(a, (int)threadIdx.x + k * GN_THREADS < nparts ? x[k] : 0.0);
    a = gn_block_reduce<INF>(a);
    if (threadIdx.x == 0) {
        // torch: clamp(max_norm / (norm + 1e-6), max = 1) on an fp32 tensor, where scalar / tensor is tensor.reciprocal() * scalar --
        // the same three fp32 roundings here.  The reciprocal goes through double (the library builds with -ffast-math: an fp32 1 / x
        // is v_rcp_f32, up to 1 ulp off; a double quotient rounded to fp32 is the IEEE fp32 quotient -- torch's device reciprocal was
        // measured up to 1 ulp away from it, tests/test_clip_gpu.py)
        const float norm = (float)((INF ? a : sqrt(a)) * fabs(gscale));
        float c = (float)(1.0 / (double)(norm + 1e-6f)) * max_norm;
        c = c > 1.f ? 1.f : c;
        out[0] = norm;
        out[1] = c;
        out[2] = (float)((double)c * gscale);
    }
}

// g[seg] *= *coef over the same segment list (the torch-semantics clip_grad_norm_ drop-in: it scales .grad in place)
__global__ __launch_bounds__(GN_THREADS) void grad_scale_kernel(float* __restrict__ g, size_t n, const long long* __restrict__ segs, int nseg,
                                                                const float* __restrict__ coef) {
    const float k = *coef;
    const size_t T = (size_t)gridDim.x * GN_THREADS, t = (size_t)blockIdx.x * GN_THREADS + threadIdx.x;
    const size_t nfull = n >> 2;
    for (int s = 0; s < nseg; ++s) {
        const size_t lo = min((size_t)segs[2 * s], n), hi = min(lo + (size_t)segs[2 * s + 1], n);
        const size_t c0 = lo >> 2, c1 = min((hi + 3) >> 2, nfull);
        for (size_t c = c0 + t; c < c1; c += GN_UNROLL * T) {
            float4 x[GN_UNROLL];
#pragma unroll
            for (int u = 0; u < GN_UNROLL; ++u) x[u] = *(const float4*)(g + 4 * min(c + u * T, c1 - 1));
#pragma unroll
            for (int u = 0; u < GN_UNROLL; ++u) {
                const size_t e = 4 * (c + u * T);
                if (c + u * T >= c1) continue;
                if (e >= lo && e + 4 <= hi) {
                    *(float4*)(g + e) = make_float4(x[u].x * k, x[u].y * k, x[u].z * k, x[u].w * k);
                } else {                                         // a float4 across a segment edge: only the segment's own elements
                    const float xs[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
#pragma unroll
                    for (int r = 0; r < 4; ++r) if (e + r >= lo && e + r < hi) g[e + r] = xs[r] * k;
                }
            }
        }
        if (t == 0 && hi > 4 * nfull && lo < hi) {               // the buffer's last partial float4 (n % 4 != 0)
            float xs[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) xs[r] = g[min(4 * nfull + r, n - 1)];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const size_t e = 4 * nfull + r;
                if (e >= lo && e < hi) g[e] = xs[r] * k;
            }
        }
    }
}

__global__ void cast_f32_bf16_kernel(const float* __restrict__ x, bf16_t* __restrict__ y, size_t n) {
    for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (size_t)gridDim.x * blockDim.x * 4) {
        const float4 a = *(const float4*)(x + i);
        bf16x4 o = {f2bf(a.x), f2bf(a.y), f2bf(a.z), f2bf(a.w)};
        *(bf16x4*)(y + i) = o;
    }
}

__global__ void cast_bf16_f32_kernel(const bf16_t* __restrict__ x, float* __restrict__ y, size_t n) {
    for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (size_t)gridDim.x * blockDim.x * 4) {
        const bf16x4 a = *(const bf16x4*)(x + i);
        *(float4*)(y + i) = make_float4(bf2f(a[0]), bf2f(a[1]), bf2f(a[2]), bf2f(a[3]));
    }
}

// du = dy * gelu'(u)   (MLM head transform, HF:476-480; the encoder's FFN fuses this into its dgrad GEMM)
__global__ void gelu_bwd_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ u, bf16_t* __restrict__ du, size_t n) {
    for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (size_t)gridDim.x * blockDim.x * 4) {
        const bf16x4 a = *(const bf16x4*)(dy + i), b = *(const bf16x4*)(u + i);
        bf16x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = f2bf(bf2f(a[r]) * gelu_erf_grad(bf2f(b[r])));
        *(bf16x4*)(du + i) = o;
    }
}

// batched transpose-cast: for each descriptor d: dst[c][r] (bf16, ld = dst_ld) = src[r][c] (fp32 or bf16 [rows, cols])
// (the bf16 source is the working copy AdamW has just written: half the bytes to read, the same values)
struct TransDesc { long long src_off, dst_off; int rows, cols, dst_ld, tile0; };
template <typename SRC>
__global__ __launch_bounds__(256) void transpose_cast_kernel(const SRC* __restrict__ src, bf16_t* __restrict__ dst,
                                                             const TransDesc* __restrict__ descs, int ndesc) {
    __shared__ float t[64][65];
    // the matrix this tile belongs to: binary search over the descriptors' first-tile numbers (a linear scan of the ~50 matrices of a
    // 12-layer model was ~25 dependent loads in front of every 16-KB tile: 150 -> 118 us per step for the search alone)
    int lo = 0, hi = ndesc - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int)blockIdx.x >= descs[mid].tile0) lo = mid; else hi = mid - 1;
    }
    const TransDesc ds = descs[lo];
    const int tl = blockIdx.x - ds.tile0;
    const int tc = (ds.cols + 63) >> 6;
    const int r0 = (tl / tc) << 6, c0 = (tl % tc) << 6;
    const SRC* s = src + ds.src_off;
    bf16_t* o = dst + ds.dst_off;
    const bool full = r0 + 64 <= ds.rows && c0 + 64 <= ds.cols && r0 + 64 <= ds.dst_ld && !(ds.cols & 3) && !(ds.dst_ld & 7) && !(ds.src_off & 3) && !(ds.dst_off & 7);
    if (full) {                                  // interior tile: 16-byte reads along a source row, 16-byte writes along a destination row
        // the thread's four reads are issued together (as a loop hipcc left it rolled: read, wait, LDS store, four times -- four
        // memory round trips per 8-KB tile; the launch took 100 us for 340 MB)
        typedef typename std::conditional<sizeof(SRC) == 4, float4, bf16x4>::type V4;
        V4 v4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = threadIdx.x + 256 * q, r = e >> 4, c = (e & 15) << 2;
            v4[q] = *(const V4*)(s + (size_t)(r0 + r) * ds.cols + c0 + c);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = threadIdx.x + 256 * q, r = e >> 4, c = (e & 15) << 2;
            if constexpr (sizeof(SRC) == 4) {
                t[r][c] = v4[q].x; t[r][c + 1] = v4[q].y; t[r][c + 2] = v4[q].z; t[r][c + 3] = v4[q].w;
            } else {
                t[r][c] = bf2f(v4[q][0]); t[r][c + 1] = bf2f(v4[q][1]); t[r][c + 2] = bf2f(v4[q][2]); t[r][c + 3] = bf2f(v4[q][3]);
            }
        }
        __syncthreads();
        for (int e = threadIdx.x; e < 512; e += 256) {
            const int c = e >> 3, r = (e & 7) << 3;
            bf16x8 ov;
#pragma unroll
            for (int j = 0; j < 8; ++j) ov[j] = f2bf(t[r + j][c]);
            *(bf16x8*)(o + (size_t)(c0 + c) * ds.dst_ld + r0 + r) = ov;
        }
        return;
    }
    for (int e = threadIdx.x; e < 4096; e += 256) {
        const int r = e >> 6, c = e & 63;
        t[r][c] = (r0 + r < ds.rows && c0 + c < ds.cols) ? (float)s[(size_t)(r0 + r) * ds.cols + c0 + c] : 0.f;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 4096; e += 256) {
        const int c = e >> 6, r = e & 63;
        if (c0 + c < ds.cols && r0 + r < ds.dst_ld) o[(size_t)(c0 + c) * ds.dst_ld + r0 + r] = f2bf(r0 + r < ds.rows ? t[r][c] : 0.f);
    }
}

// Batched row gather: dst_k[i][:] = src_k[idx[i]][:] for up to 12 matrices that share ONE row list (the sparse backward paths gather
// the same few hundred rows of every saved activation: 9 + 6 index_select launches of ~5 us per step before).  Rows are byte
// strings (row_bytes % 4 == 0, 16-byte pieces where the pointers and pitches allow); grid (rows, matrices).
struct GatherSeg { const char* src; char* dst; long long src_pitch, dst_pitch; int row_bytes, vec16; };
struct GatherArgs { GatherSeg s[12]; };
__global__ __launch_bounds__(256) void gather_rows_kernel(const GatherArgs a, const int* __restrict__ idx) {
    const GatherSeg s = a.s[blockIdx.y];
    const int i = blockIdx.x;
    const char* src = s.src + (long long)idx[i] * s.src_pitch;
    char* dst = s.dst + (long long)i * s.dst_pitch;
    if (s.vec16) {
        for (int b = threadIdx.x * 16; b < s.row_bytes; b += 256 * 16) *(uint4*)(dst + b) = *(const uint4*)(src + b);
    } else {
        for (int b = threadIdx.x * 4; b < s.row_bytes; b += 256 * 4) *(uint32_t*)(dst + b) = *(const uint32_t*)(src + b);
    }
}

// Concatenation of up to 12 int64 segments into one buffer (token ids, token types and labels of the step's passes: three
// torch.cat launches, two zero fills and their dtype conversions before); a segment without a source is filled with a constant.
struct PackSeg { const int64_t* src; long long dst0, n, fill; };
struct PackArgs { PackSeg s[12]; };
__global__ __launch_bounds__(256) void pack_i64_kernel(const PackArgs a, int64_t* __restrict__ out) {
    const PackSeg s = a.s[blockIdx.y];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < s.n; i += (long long)gridDim.x * 256)
        out[s.dst0 + i] = s.src ? s.src[i] : (int64_t)s.fill;
}

// test/debug: keep mask of a dropout site as bytes (so the CPU oracle can replay the same mask)
__global__ void dropout_mask_kernel(uint8_t* __restrict__ out, size_t n, uint32_t stream, uint32_t thr) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = mmb_keep(stream, i, thr) ? 1 : 0;
}

// MLM masking on the device (REF:model_utils.py:6-39): element i draws ONE 32-bit word from the counter RNG; its low half decides
// "selected" (probability sel_thr16 / 65536, never for the special ids), its high half "replaced by [MASK]" (rep_thr16 / 65536 of
// the selected).  labels[i] = the original id where selected, -100 elsewhere; ids are rewritten in place like the reference does.
__global__ void mlm_mask_kernel(int64_t* __restrict__ ids, int64_t* __restrict__ labels, size_t n, uint32_t stream, uint32_t sel_thr16,
                                uint32_t rep_thr16, int64_t special0, int64_t special1, int64_t special2, int64_t mask_id) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int64_t id = ids[i];
        const uint32_t h = mmb_pair_bits(stream, (uint32_t)i);
        const bool special = (id == special0) | (id == special1) | (id == special2);
        const bool sel = !special && (h & 0xFFFFu) < sel_thr16;
        labels[i] = sel ? id : (int64_t)-100;
        if (sel && (h >> 16) < rep_thr16) ids[i] = mask_id;
    }
}


// --------------------------------------------------------------------------------------------
// Step prologue: from the caller's attention masks and MLM labels to everything the encoder's launches need, in TWO launches
// (round 1 spent ~45 element-wise torch launches and two device->host copies on this: 0.8 ms of a 17.5 ms step).
//   A (one workgroup per sequence): the padded additive key bias (REF:MMBertForPretraining.py:57-154: (1 - mask) * -10000 per key,
//     -1e30 in the padding slots), kv_len (keys behind it are all masked out: attn_kv_len_kernel's rule), valid = max(kv_len, last
//     labelled position + 1) (the rows backward must visit: model._split_layout), and per-sequence label counts;
//   B (one workgroup per sequence): the ascending list of labelled rows (mmbert_active_rows' output) and the host words
//     [valid[0..nseq), #labelled rows, #labelled first rows, #labels outside {-100} u [0, V)] -- ONE device->host copy.
// A mask segment = positions [offset, offset + len) of every sequence of one pass, element (b, p) at ptr + b*sb + p*sp bytes, any of
// the dtypes the reference's collate produces (float64 / int64) or torch hands over.
// --------------------------------------------------------------------------------------------
struct MaskSeg { const char* ptr; long long sb, sp; int dtype, pass, offset, len; };
#define PRO_MAXSEG 12
#define PRO_MAXPASS 4
struct PrologueArgs {
    MaskSeg seg[PRO_MAXSEG];
    int nseg, npass, B, vocab;
    int pass_len[PRO_MAXPASS], pass_row0[PRO_MAXPASS], pass_bias0[PRO_MAXPASS];
    const int64_t* labels;
    float* key_bias; int* kv_len; int* valid; int* seq_cnt;      // seq_cnt: [3][nseq] labelled rows / labelled first row / bad labels
    int* idx; int* words;
    // row-set mode (both or neither): rank[row] = position of the row in its sequence's valid-first order, key_bias_perm = the padded
    // key bias in that order; valid[s] then COUNTS the active rows (unmasked key, or labelled) instead of bounding a prefix
    int* rank; float* key_bias_perm;
};

__device__ __forceinline__ float mask_value(const MaskSeg& g, int b, int p) {
    const char* a = g.ptr + (long long)b * g.sb + (long long)p * g.sp;
    switch (g.dtype) {
        case 0: return *(const float*)a;
        case 1: return (float)*(const double*)a;
        case 2: return (float)*(const int64_t*)a;
        case 3: return (float)*(const int*)a;
        case 4: return bf2f(*(const bf16_t*)a);
        case 5: return (float)*(const uint8_t*)a;
        default: return (float)*(const _Float16*)a;
    }
}

// (1 - m) * -10000 with the reference's two fp32 roundings.  Written as plain operators, -ffast-math let hipcc distribute it into ONE
// fma(m, 10000, -10000): one rounding, so m = 3e-8 read as a masked key (-10000) where the reference's -9999.999 is a live one, and
// m = 1 gave +0 where the reference gives -0.  The round-to-nearest library forms are never reassociated or contracted.
__device__ __forceinline__ float key_bias_of(float m) { return __ocml_mul_rte_f32(__ocml_sub_rte_f32(1.0f, m), -10000.0f); }

__global__ __launch_bounds__(256) void prologue_seq_kernel(const PrologueArgs a) {
    __shared__ int red[4][5];
    const int s = blockIdx.x, p = s / a.B, b = s - p * a.B;
    const int S = a.pass_len[p], row0 = a.pass_row0[p] + b * S;
    const int slots = (S + 127) & ~127;
    float* kb = a.key_bias + a.pass_bias0[p] + b * slots;
    int last_key = -1, last_lab = -1, cnt = 0, first = 0, bad = 0;
    for (int pos = threadIdx.x; pos < slots; pos += 256) {
        float bias = -1.0e30f;
        if (pos < S) {
            float m = 1.0f;
            for (int q = 0; q < a.nseg; ++q) {
                const MaskSeg& g = a.seg[q];
                if (g.pass == p && pos >= g.offset && pos < g.offset + g.len) { m = mask_value(g, b, pos - g.offset); break; }
            }
            bias = key_bias_of(m);
            if (bias > -10000.0f) last_key = pos;
            if (a.labels) {
                const int64_t lab = a.labels[row0 + pos];
                if (lab != -100) {
                    last_lab = pos;
                    if (lab >= 0 && lab < a.vocab) { ++cnt; if (pos == 0) first = 1; } else ++bad;
                }
            }
        }
        kb[pos] = bias;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        last_key = max(last_key, __shfl_xor(last_key, o, 64)); last_lab = max(last_lab, __shfl_xor(last_lab, o, 64));
        cnt += __shfl_xor(cnt, o, 64); first += __shfl_xor(first, o, 64); bad += __shfl_xor(bad, o, 64);
    }
    if (lane == 0) { red[w][0] = last_key; red[w][1] = last_lab; red[w][2] = cnt; red[w][3] = first; red[w][4] = bad; }
    __syncthreads();
    __shared__ int all_active;
    if (threadIdx.x == 0) {
        const int nseq = a.npass * a.B;
        int lk = -1, ll = -1, c = 0, f = 0, bd = 0;
        for (int q = 0; q < 4; ++q) { lk = max(lk, red[q][0]); ll = max(ll, red[q][1]); c += red[q][2]; f += red[q][3]; bd += red[q][4]; }
        const int kv = lk < 0 ? S : lk + 1;                     // no unmasked key at all: the sequence keeps its full length
        a.kv_len[s] = kv;
        if (!a.rank) a.valid[s] = max(kv, ll + 1);
        a.seq_cnt[s] = c; a.seq_cnt[nseq + s] = f; a.seq_cnt[2 * nseq + s] = bd;
        all_active = lk < 0;
    }
    if (!a.rank) return;
    // ---- row-set mode: a row is ACTIVE iff it is an unmasked key or carries a label (a query with a gradient); the active rows of the
    // sequence come first, both groups keep their order.  Two sweeps over the positions: count, then place (ballot prefix sums).
    __shared__ int wcount[4];
    __shared__ int nact_s;
    __syncthreads();                                               // kb[] of this sequence (pass 1) and all_active are visible
    const bool every = all_active != 0;
    auto active = [&](int pos) {                                   // position 0 always: the heads read the [CLS] row of every sequence
        if (every || pos == 0 || kb[pos] > -10000.0f) return true;
        return a.labels && a.labels[row0 + pos] != -100;
    };
    int mine = 0;
    for (int pos = threadIdx.x; pos < S; pos += 256) mine += active(pos) ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if (lane == 0) wcount[w] = mine;
    __syncthreads();
    if (threadIdx.x == 0) { nact_s = wcount[0] + wcount[1] + wcount[2] + wcount[3]; a.valid[s] = nact_s; }
    __syncthreads();
    const int nact = nact_s;
    float* kp = a.key_bias_perm + a.pass_bias0[p] + b * slots;
    int base = 0;                                                  // active rows before this chunk
    for (int p0 = 0; p0 < slots; p0 += 256) {
        const int pos = p0 + threadIdx.x;
        const bool in = pos < S, act = in && active(pos);
        const unsigned long long bal = __ballot(act);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        __syncthreads();
        if (lane == 0) wcount[w] = __popcll(bal);
        __syncthreads();
        int off = base;
        for (int q = 0; q < w; ++q) off += wcount[q];
        if (in) {
            const int ab = off + before;                           // active rows in front of this position
            const int np = act ? ab : nact + (pos - ab);
            a.rank[row0 + pos] = np;
            kp[np] = kb[pos];
        } else if (pos < slots) {
            kp[pos] = -1.0e30f;
        }
        base += wcount[0] + wcount[1] + wcount[2] + wcount[3];
    }
}

__global__ __launch_bounds__(256) void prologue_rows_kernel(const PrologueArgs a) {
    __shared__ int wsum[4];
    __shared__ int base_s;
    const int s = blockIdx.x, p = s / a.B, b = s - p * a.B, nseq = a.npass * a.B;
    const int S = a.pass_len[p], row0 = a.pass_row0[p] + b * S;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) {
        int off = 0;
        for (int q = 0; q < s; ++q) off += a.seq_cnt[q];
        base_s = off;
        a.words[s] = a.valid[s];
        if (s == 0) {
            int t0 = 0, t1 = 0, t2 = 0;
            for (int q = 0; q < nseq; ++q) { t0 += a.seq_cnt[q]; t1 += a.seq_cnt[nseq + q]; t2 += a.seq_cnt[2 * nseq + q]; }
            a.words[nseq] = t0; a.words[nseq + 1] = t1; a.words[nseq + 2] = t2;
        }
    }
    __syncthreads();
    if (!a.labels || a.seq_cnt[s] == 0) return;
    int base = base_s;
    for (int p0 = 0; p0 < S; p0 += 256) {
        const int pos = p0 + tid;
        bool act = false;
        if (pos < S) { const int64_t lab = a.labels[row0 + pos]; act = lab >= 0 && lab < a.vocab; }
        const unsigned long long bal = __ballot(act);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        __syncthreads();
        if (lane == 0) wsum[w] = __popcll(bal);
        __syncthreads();
        int off = base;
        for (int q = 0; q < w; ++q) off += wsum[q];
        if (act) a.idx[off + before] = row0 + pos;
        base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    }
}

// Compact exchange of embedding-row gradients (data parallel, parallel.exchange_rows): block[pos(ids[i])] += rows[i], pos = the index of
// ids[i] in the ascending list `uni` (the union of touched table rows over all ranks); ids outside (0, V) or not in the list carry
// nothing.  One workgroup per row, the binary search is wave-uniform; rows bf16 or fp32.  (Round 3: eleven ATen launches before.)
__global__ __launch_bounds__(256) void rows_to_block_kernel(const int64_t* __restrict__ ids, const void* __restrict__ rows, int rows_bf16, int ldr,
                                                            int n, int H, const int64_t* __restrict__ uni, int U, int V, float* __restrict__ block) {
    const int i = blockIdx.x;
    if (i >= n || U <= 0) return;
    const long long id = ids[i];
    if (id <= 0 || id >= V) return;
    int lo = 0, hi = U - 1;
    while (lo < hi) {                                          // first position with uni[pos] >= id
        const int mid = (lo + hi) >> 1;
        if (uni[mid] < id) lo = mid + 1; else hi = mid;
    }
    if (uni[lo] != id) return;
    float* dst = block + (size_t)lo * H;
    for (int c = threadIdx.x; c < H; c += 256) {
        const float v = rows_bf16 ? bf2f(((const bf16_t*)rows)[(size_t)i * ldr + c]) : ((const float*)rows)[(size_t)i * ldr + c];
        atomicAdd(dst + c, v);
    }
}

template <typename FT>
static int pair_proj_fwd_launch(hipStream_t stream, const FT* feat, int n, int P, int D, const float* W, const float* bias, int H, void* out, int ldo, int T,
                                int KC, int pitch, int lds) {
    static std::atomic<unsigned long long> attr_done{0};
    if (KC <= 64) {                                                // 64 lanes of k per row (four rows per wave-instruction pair) or 128
        hipLaunchKernelGGL((pair_proj_fwd_kernel<6, FT>), dim3((n + 63) / 64, (H + 127) / 128), dim3(256), lds, stream, feat, n, P, D, W, bias, H, (bf16_t*)out, ldo, T,
                           KC, pitch);
    } else {
        if (int e = mmb_allow_lds((const void*)pair_proj_fwd_kernel<7, FT>, 192 * 130 * (int)sizeof(float), attr_done)) return e;
        hipLaunchKernelGGL((pair_proj_fwd_kernel<7, FT>), dim3((n + 63) / 64, (H + 127) / 128), dim3(256), lds, stream, feat, n, P, D, W, bias, H, (bf16_t*)out, ldo, T,
                           KC, pitch);
    }
    MMB_CHECK_LAUNCH();
    return 0;
}

extern "C" {

uint32_t mmbert_rng_stream(uint64_t seed, uint32_t site) {
    uint32_t a = mmb_hash32((uint32_t)seed ^ 0xA511E9B3u);
    uint32_t b = mmb_hash32((uint32_t)(seed >> 32) + 0x7F4A7C15u);
    return mmb_hash32(a ^ (b * 0x9E3779B1u) ^ mmb_hash32(site * 0x85EBCA6Bu + 0x27D4EB2Fu));
}

uint32_t mmbert_dropout_thr16(float p) {
    if (p <= 0.f) return 0;
    double t = (double)p * 65536.0 + 0.5;
    if (t > 65535.0) t = 65535.0;
    return (uint32_t)t;
}

int mmbert_embed_gather(hipStream_t stream, const int64_t* ids, const int64_t* tts, const float* word, const float* type, const float* pos,
                        int n, int T, int H, int V, void* out, int ldo) {
    if (n <= 0) return 0;
    if ((H & 3) || (ldo & 3)) return -1;
    hipLaunchKernelGGL(embed_gather_kernel, dim3(grid_for(n, 4)), dim3(256), 0, stream, ids, tts, word, type, pos, n, T, H, V, (bf16_t*)out, ldo);
    MMB_CHECK_LAUNCH();
    return 0;
}

int mmbert_embed_scatter(hipStream_t stream, const int64_t* ids, const int64_t* tts, const void* d, int ldd, int n, int T, int H, int V,
                         float* gword, float* gtype, float* gpos, float* type_slab) {
    if (n <= 0) return 0;
    if (H > LN_MAXV * 256 || (H & 3) || (ldd & 3) || T <= 0) return -1;
    // deterministic mode: the word rows cannot come from this kernel (a word at several positions: atomics in arrival order -- the caller
    // uses mmbert_id_runs_sum_rows) and the token-type sums need the slab (2 * T * H floats)
    if (mmb_deterministic() && (gword != nullptr || type_slab == nullptr)) return -4;
    constexpr int slices = 1;   // grid.y slices of the sequences; measured at the headline shape: 1 / 2 / 4 / 8 = 37.8 / 39.1 / 49.0 / 59.2 us (same-address atomics on the two token-type rows)
    hipLaunchKernelGGL(embed_scatter_kernel, dim3(T < n ? T : n, slices), dim3(256), 0, stream, ids, tts, (const bf16_t*)d, ldd, n, T, H, V, gword, gtype, gpos, type_slab);
    MMB_CHECK_LAUNCH();
    if (type_slab) {
        hipLaunchKernelGGL(embed_type_fold_kernel, dim3((2 * H + 255) / 256), dim3(256), 0, stream, type_slab, T < n ? T : n, H, gtype);
        MMB_CHECK_LAUNCH();
    }
    return 0;
}

int mmbert_pair_proj_fwd(hipStream_t stream, const void* feat, int feat_f64, int B, int P, int D, const float* W, const float* bias, int H,
                         void* out, int ldo, int T) {
    const int n = B * P;
    if (n <= 0) return 0;
    if (D < 1 || H < 1) return -1;
    const int KC = D < 128 ? (D + 3) & ~3 : 128;                 // k chunk in LDS (a multiple of 4); row pitch = 2 mod 16 floats
    const int pitch = KC + ((18 - (KC & 15)) & 15);
    // the operand tiles, and the output tile the full-tile store stages through the same LDS ([64][136] bf16: 17 408 bytes, more
    // than the operand tiles of D <= 16 take -- rows 51-63 of every such tile were lost)
    const int ops_lds = 192 * pitch * (int)sizeof(float), out_lds = 64 * 136 * (int)sizeof(bf16_t);
    const int lds = ops_lds > out_lds ? ops_lds : out_lds;       // <= 99 840 bytes
    return feat_f64 ? pair_proj_fwd_launch(stream, (const double*)feat, n, P, D, W, bias, H, out, ldo, T, KC, pitch, lds)
                    : pair_proj_fwd_launch(stream, (const float*)feat, n, P, D, W, bias, H, out, ldo, T, KC, pitch, lds);
}

// workspace: the slab [S][H][D + 1] fp32 of per-row-range partial products.  S row ranges (a multiple of 16 rows each) so that the
// launch has about one workgroup per CU, i.e. one wave per SIMD: twenty independent accumulators keep the matrix pipe busy from one wave
static void pair_bwd_split(int n, int D, int H, int* rows_per_wg, int* S) {
    const int htiles = (H + 63) / 64, zt = ((D + 1 + 15) / 16 + PAIR_NT - 1) / PAIR_NT;
    int want = (mmb_device_cus() + htiles * zt - 1) / (htiles * zt);
    if (want < 1) want = 1;
    int rp = ((n + want - 1) / want + 63) / 64 * 64;             // a multiple of 64: 16 per wave and ring turn
    if (rp < 64) rp = 64;
    *rows_per_wg = rp;
    *S = (n + rp - 1) / rp;
}
size_t mmbert_pair_proj_bwd_workspace(int B, int P, int D, int H) {
    if (B <= 0 || P <= 0 || D < 1 || H < 1) return 0;
    int rp, S;
    pair_bwd_split(B * P, D, H, &rp, &S);
    return (size_t)S * H * (D + 1) * sizeof(float);
}

int mmbert_pair_proj_bwd(hipStream_t stream, const void* feat, int feat_f64, int B, int P, int D, const void* J, const void* dJ, int ld, int T,
                         float* dW, float* db, int H, void* workspace) {
    const int n = B * P;
    if (n <= 0) return 0;
    if (!workspace || (H & 7) || (ld & 7) || D < 1) return -1;
    PairBwdArgs a = {};
    a.feat = feat; a.J = (const bf16_t*)J; a.dJ = (const bf16_t*)dJ; a.slab = (float*)workspace;
    a.n = n; a.P = P; a.D = D; a.T = T; a.H = H; a.ld = ld;
    int S;
    pair_bwd_split(n, D, H, &a.rows_per_wg, &S);
    a.ntiles = (D + 1 + 15) / 16;
    const dim3 grid((H + 63) / 64, S, (a.ntiles + PAIR_NT - 1) / PAIR_NT);
    if (feat_f64) hipLaunchKernelGGL(pair_wgrad_kernel<double>, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(pair_wgrad_kernel<float>, grid, dim3(256), 0, stream, a);
    MMB_CHECK_LAUNCH();
    hipLaunchKernelGGL(pair_wgrad_reduce_kernel, dim3((H * (D + 1) + 255) / 256), dim3(256), 0, stream, (const float*)workspace, S, H, D, dW, db);
    MMB_CHECK_LAUNCH();
    return 0;
}

// label smoothing of the _smooth entry points: inside [0, 1) and finite, or nothing is launched
static bool ce_smoothing_ok(float smoothing) { return smoothing >= 0.f && smoothing < 1.f; }      // (false for a NaN)

static int ce_fwd_launch(hipStream_t stream, const void* logits, int ldv, int V, const int64_t* labels, int M, const int* seg_bounds, int nseg,
                         float* inv_count, float* loss_sum, float* row_lse, int logits_f32, float* row_loss, float smoothing) {
    if (M <= 0) return 0;
    if (nseg < 1 || nseg > 4 || (ldv & 7) || ldv > CE_MAXC * 256 * 8 || V > ldv) return -1;
    if (smoothing != 0.f && V < 1) return -1;                     // (eps / V)
    const bool det = mmb_deterministic();
    if (det && !row_loss) return -4;                              // deterministic mode needs the per-row loss buffer (M floats)
    if (!det) row_loss = nullptr;
    hipLaunchKernelGGL(ce_count_kernel, dim3(1), dim3(1024), 0, stream, labels, M, V, seg_bounds, nseg, inv_count, loss_sum);
    MMB_CHECK_LAUNCH();
    if (smoothing != 0.f) {
        const float one_minus = 1.f - smoothing, eps_over_v = smoothing / (float)V;
        if (logits_f32)
            hipLaunchKernelGGL((ce_row_kernel<0, true, true>), dim3(M), dim3(256), 0, stream, logits, ldv, V, labels, seg_bounds, nseg, inv_count,
                               loss_sum, row_lse, (const float*)nullptr, (bf16_t*)nullptr, 0, (const int*)nullptr, row_loss, one_minus, eps_over_v);
        else
            hipLaunchKernelGGL((ce_row_kernel<0, false, true>), dim3(M), dim3(256), 0, stream, logits, ldv, V, labels, seg_bounds, nseg, inv_count,
                               loss_sum, row_lse, (const float*)nullptr, (bf16_t*)nullptr, 0, (const int*)nullptr, row_loss, one_minus, eps_over_v);
    } else if (logits_f32)
        hipLaunchKernelGGL((ce_row_kernel<0, true>), dim3(M), dim3(256), 0, stream, logits, ldv, V, labels, seg_bounds, nseg, inv_count, loss_sum,
                           row_lse, (const float*)nullptr, (bf16_t*)nullptr, 0, (const int*)nullptr, row_loss, 1.f, 0.f);
    else
        hipLaunchKernelGGL((ce_row_kernel<0, false>), dim3(M), dim3(256), 0, stream, logits, ldv, V, labels, seg_bounds, nseg, inv_count, loss_sum,
                           row_lse, (const float*)nullptr, (bf16_t*)nullptr, 0, (const int*)nullptr, row_loss, 1.f, 0.f);
    MMB_CHECK_LAUNCH();
    if (det) {
        hipLaunchKernelGGL(ce_loss_sum_ordered_kernel, dim3(1), dim3(1024), 0, stream, (const float*)row_loss, M, seg_bounds, nseg, loss_sum);
        MMB_CHECK_LAUNCH();
    }
    return 0;
}

int mmbert_ce_fwd(hipStream_t stream, const void* logits, int ldv, int V, const int64_t* labels, int M,
                  const int* seg_bounds, int nseg, float* inv_count, float* loss_sum, float* row_lse, int logits_f32, float* row_loss) {
    return ce_fwd_launch(stream, logits, ldv, V, labels, M, seg_bounds, nseg, inv_count, loss_sum, row_lse, logits_f32, row_loss, 0.f);
}

int mmbert_ce_fwd_smooth(hipStream_t stream, const void* logits, int ldv, int V, const int64_t* labels, int M, const int* seg_bounds, int nseg,
                         float* inv_count, float* loss_sum, float* row_lse, int logits_f32, float* row_loss, float smoothing) {
    if (!ce_smoothing_ok(smoothing)) return -1;
    return ce_fwd_launch(stream, logits, ldv, V, labels, M, seg_bounds, nseg, inv_count, loss_sum, row_lse, logits_f32, row_loss, smoothing);
}

int mmbert_vocab_topk(hipStream_t stream, const void* logits, int ldv, int V, int M, int logits_f32, int k, const int64_t* labels,
                      int32_t* top_ids, float* top_logprob, float* row_lse, float* label_logprob, int32_t* label_rank) {
    if (M < 0 || V < 1 || V > CE_MAXC * 256 * 8 || k < 1 || k > 8 || k > V || (ldv & 7) || ldv < V) return -1;
    if (M == 0) return 0;                                          // (an empty tensor has no address)
    if (!logits || !top_ids || !top_logprob || !row_lse) return -1;
    if (labels ? (!label_logprob || !label_rank) : (label_logprob || label_rank)) return -1;
    if (logits_f32)
        hipLaunchKernelGGL(vocab_topk_kernel<true>, dim3(M), dim3(256), 0, stream, logits, ldv, V, k, labels, top_ids, top_logprob, row_lse,
                           label_logprob, label_rank);
    else
        hipLaunchKernelGGL(vocab_topk_kernel<false>, dim3(M), dim3(256), 0, stream, logits, ldv, V, k, labels, top_ids, top_logprob, row_lse,
                           label_logprob, label_rank);
    MMB_CHECK_LAUNCH();
    return 0;
}

void mmbert_set_deterministic(int on) { g_mmb_deterministic.store(on != 0); }
int mmbert_get_deterministic(void) { return g_mmb_deterministic.load(); }

int mmbert_id_runs_sum_rows(hipStream_t stream, const void* src, int src_bf16, int lds, const int64_t* ids, int n,
                            int H, int V, const int64_t* uni, int U, float* dst, int ldd) {
    if (n <= 0) return 0;
    if ((H & 3) || H > 4096 || n > RUNS_MAXN || (lds & 3) || (ldd & 3) || !src || !ids || !dst) return -1;
    const int CT = H >> 2;
    int G = 1024 / CT; if (G > 8) G = 8; if (G < 1) G = 1;
    int threads = G * CT; if (threads < 64) threads = 64;
    hipLaunchKernelGGL(id_runs_sum_rows_kernel, dim3(n), dim3(threads), 0, stream, src, src_bf16, lds, ids, n, H, V, uni, U, dst, ldd);
    MMB_CHECK_LAUNCH();
    return 0;
}

static int ce_bwd_launch(hipStream_t stream, const void* logits, int ldv, int V, const int64_t* labels, int M, const int* seg_bounds, int nseg,
                         const float* inv_count, const float* gscale, const float* row_lse, void* dlogits, int ldd, const int* rows, int nrows,
                         int logits_f32, float smoothing) {
    if (M <= 0 || (rows && nrows <= 0)) return 0;
    if (nseg < 1 || nseg > 4 || (ldv & 7) || (ldd & 7) || ldv > CE_MAXC * 256 * 8 || V > ldv) return -1;
    if (smoothing != 0.f && V < 1) return -1;
    if (smoothing != 0.f) {
        const float one_minus = 1.f - smoothing, eps_over_v = smoothing / (float)V;
        if (logits_f32)
            hipLaunchKernelGGL((ce_row_kernel<1, true, true>), dim3(rows ? nrows : M), dim3(256), 0, stream, logits, ldv, V, labels, seg_bounds, nseg,
                               inv_count, (float*)nullptr, (float*)row_lse, gscale, (bf16_t*)dlogits, ldd, rows, (float*)nullptr, one_minus, eps_over_v);
        else
            hipLaunchKernelGGL((ce_row_kernel<1, false, true>), dim3(rows ? nrows : M), dim3(256), 0, stream, logits, ldv, V, labels, seg_bounds, nseg,
                               inv_count, (float*)nullptr, (float*)row_lse, gscale, (bf16_t*)dlogits, ldd, rows, (float*)nullptr, one_minus, eps_over_v);
    } else if (logits_f32)
        hipLaunchKernelGGL((ce_row_kernel<1, true>), dim3(rows ? nrows : M), dim3(256), 0, stream, logits, ldv, V, labels, seg_bounds, nseg, inv_count,
                           (float*)nullptr, (float*)row_lse, gscale, (bf16_t*)dlogits, ldd, rows, (float*)nullptr, 1.f, 0.f);
    else
        hipLaunchKernelGGL((ce_row_kernel<1, false>), dim3(rows ? nrows : M), dim3(256), 0, stream, logits, ldv, V, labels, seg_bounds, nseg, inv_count,
                           (float*)nullptr, (float*)row_lse, gscale, (bf16_t*)dlogits, ldd, rows, (float*)nullptr, 1.f, 0.f);
    MMB_CHECK_LAUNCH();
    return 0;
}

int mmbert_ce_bwd(hipStream_t stream, const void* logits, int ldv, int V, const int64_t* labels, int M,
                  const int* seg_bounds, int nseg, const float* inv_count, const float* gscale, const float* row_lse, void* dlogits, int ldd,
                  const int* rows, int nrows, int logits_f32) {
    return ce_bwd_launch(stream, logits, ldv, V, labels, M, seg_bounds, nseg, inv_count, gscale, row_lse, dlogits, ldd, rows, nrows, logits_f32, 0.f);
}

int mmbert_ce_bwd_smooth(hipStream_t stream, const void* logits, int ldv, int V, const int64_t* labels, int M, const int* seg_bounds, int nseg,
                         const float* inv_count, const float* gscale, const float* row_lse, void* dlogits, int ldd, const int* rows, int nrows,
                         int logits_f32, float smoothing) {
    if (!ce_smoothing_ok(smoothing)) return -1;
    return ce_bwd_launch(stream, logits, ldv, V, labels, M, seg_bounds, nseg, inv_count, gscale, row_lse, dlogits, ldd, rows, nrows, logits_f32,
                         smoothing);
}

int mmbert_split_rows(hipStream_t stream, const int64_t* row_seq, const int64_t* row_pos, const int* start_a, const int* start_b, const int* valid,
                      int mode, int M, int rows_a, int64_t* perm, int64_t* inv, const int* rank, int* perm32, int* inv32) {
    if (M <= 0) return 0;
    if (mode < 0 || mode > 2) return -1;
    hipLaunchKernelGGL(split_rows_kernel, dim3((M + 255) / 256), dim3(256), 0, stream, row_seq, row_pos, start_a, start_b, valid, mode, M, rows_a, perm, inv, rank,
                       perm32, inv32);
    MMB_CHECK_LAUNCH();
    return 0;
}

int mmbert_split_layout(hipStream_t stream, const int* seq_len, const int* valid, int nseq, int tile_rows, int xs, int nf_max, int nq_max, int* out) {
    if (nseq <= 0) return 0;
    if (nseq > SL_MAXSEQ || tile_rows <= 0 || xs <= 0 || !out) return -1;
    hipLaunchKernelGGL(split_layout_kernel, dim3(1), dim3(1024), 0, stream, seq_len, valid, nseq, tile_rows, xs, nf_max, nq_max, out);
    MMB_CHECK_LAUNCH();
    return 0;
}

int mmbert_prologue(hipStream_t stream, int nseg, const void* const* seg_ptr, const long long* seg_stride_b, const long long* seg_stride_p,
                    const int* seg_dtype, const int* seg_pass, const int* seg_offset, const int* seg_len,
                    int npass, const int* pass_len, int B, const int64_t* labels, int vocab,
                    float* key_bias, int* kv_len, int* valid, int* seq_cnt, int* idx, int* words, int* rank, float* key_bias_perm) {
    if (npass <= 0 || B <= 0) return 0;
    if (nseg < 0 || nseg > PRO_MAXSEG || npass > PRO_MAXPASS || ((rank == nullptr) != (key_bias_perm == nullptr))) return -1;
    PrologueArgs a = {};
    for (int q = 0; q < nseg; ++q) {
        if (seg_dtype[q] < 0 || seg_dtype[q] > 6 || seg_pass[q] < 0 || seg_pass[q] >= npass) return -1;
        a.seg[q].ptr = (const char*)seg_ptr[q]; a.seg[q].sb = seg_stride_b[q]; a.seg[q].sp = seg_stride_p[q];
        a.seg[q].dtype = seg_dtype[q]; a.seg[q].pass = seg_pass[q]; a.seg[q].offset = seg_offset[q]; a.seg[q].len = seg_len[q];
    }
    int row = 0, slot = 0;
    for (int p = 0; p < npass; ++p) {
        a.pass_len[p] = pass_len[p]; a.pass_row0[p] = row; a.pass_bias0[p] = slot;
        row += B * pass_len[p]; slot += B * ((pass_len[p] + 127) & ~127);
    }
    a.nseg = nseg; a.npass = npass; a.B = B; a.vocab = vocab; a.labels = labels;
    a.key_bias = key_bias; a.kv_len = kv_len; a.valid = valid; a.seq_cnt = seq_cnt; a.idx = idx; a.words = words;
    a.rank = rank; a.key_bias_perm = key_bias_perm;
    hipLaunchKernelGGL(prologue_seq_kernel, dim3(npass * B), dim3(256), 0, stream, a);
    MMB_CHECK_LAUNCH();
    hipLaunchKernelGGL(prologue_rows_kernel, dim3(npass * B), dim3(256), 0, stream, a);
    MMB_CHECK_LAUNCH();
    return 0;
}

int mmbert_active_rows(hipStream_t stream, const int64_t* labels, int M, int V, int* idx, int* count) {
    if (M < 0) return -1;
    hipLaunchKernelGGL(active_rows_kernel, dim3(1), dim3(1024), 0, stream, labels, M, V, idx, count);
    MMB_CHECK_LAUNCH();
    return 0;
}

// The coefficients of one (lr, beta1, beta2, eps, weight_decay) at a step: every derived value in double, rounded to fp32 once (the
// reference's optimizer computes them as Python floats).
static AdamWCoefs adamw_coefs(double lr, double beta1, double beta2, double eps, double wd, int step, int mode) {
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    const double step_size = mode == 0 ? lr * sqrt(bc2) / bc1 : lr / bc1;
    return {(float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, (float)step_size, (float)(1.0 / sqrt(bc2)),
            (float)(lr * wd)};
}

// hyper[5 k ..] = (lr, beta1, beta2, eps, weight_decay) of group k -> the table of distinct combinations, in first-seen order, and
// every group's slot in it; coefs(h) forms one combination's coefficients (AdamWSlots and LambSlots share the layout of the slot words).
// -1: no hyper, ngroups outside 1 .. ADAMW_MAX_GROUPS, or more than ADAMW_MAX_SLOTS distinct combinations.
extern "C++" template <class Slots, class Coefs>
static int fill_slots(Slots& a, const double* hyper, int ngroups, Coefs coefs) {
    if (!hyper || ngroups < 1 || ngroups > ADAMW_MAX_GROUPS) return -1;
    memset(&a, 0, sizeof(a));
    const double* key[ADAMW_MAX_SLOTS];  // the first group of each slot
    int nslot = 0;
    for (int k = 0; k < ngroups; ++k) {
        const double* h = hyper + 5 * k;
        int s = 0;
        while (s < nslot && !(key[s][0] == h[0] && key[s][1] == h[1] && key[s][2] == h[2] && key[s][3] == h[3] && key[s][4] == h[4])) ++s;
        if (s == nslot) {
            if (nslot == ADAMW_MAX_SLOTS) return -1;
            key[nslot++] = h;
            a.c[s] = coefs(h);
        }
        a.slot4[k >> 2] |= (uint32_t)s << ((k & 3) * 8);
    }
    return 0;
}

static int adamw_fill_slots(AdamWSlots& a, const double* hyper, int ngroups, int step, int mode) {
    return fill_slots(a, hyper, ngroups, [&](const double* h) { return adamw_coefs(h[0], h[1], h[2], h[3], h[4], step, mode); });
}

static dim3 adamw_grid(size_t n) { return dim3((unsigned)((n / 4 + 255) / 256)); }

int mmbert_adamw(hipStream_t stream, float* p, float* g, float* m, float* v, void* p_bf16, const uint8_t* flags, size_t n,
                 double lr, double beta1, double beta2, double eps, double wd, int step, double gscale, int mode, int zero_grad) {
    if (n == 0) return 0;
    if (n & 255) return -1;
    const AdamWCoefs c = adamw_coefs(lr, beta1, beta2, eps, wd, step, mode);
    hipLaunchKernelGGL(adamw_kernel, adamw_grid(n), dim3(256), 0, stream, p, g, m, v, (bf16_t*)p_bf16, flags, n,
                       c.beta1, c.beta2, c.omb1, c.omb2, c.eps, c.step_size, c.rsbc2, c.lrwd, (float)gscale, mode, zero_grad);
    MMB_CHECK_LAUNCH();
    return 0;
}

int mmbert_adamw_devscale(hipStream_t stream, float* p, float* g, float* m, float* v, void* p_bf16, const uint8_t* flags, size_t n,
                          double lr, double beta1, double beta2, double eps, double wd, int step, const float* coef, int mode, int zero_grad) {
    if (n == 0) return 0;
    if ((n & 255) || !coef) return -1;
    const AdamWCoefs c = adamw_coefs(lr, beta1, beta2, eps, wd, step, mode);
    hipLaunchKernelGGL(adamw_devscale_kernel, adamw_grid(n), dim3(256), 0, stream, p, g, m, v, (bf16_t*)p_bf16, flags, n,
                       c.beta1, c.beta2, c.omb1, c.omb2, c.eps, c.step_size, c.rsbc2, c.lrwd, coef, mode, zero_grad);
    MMB_CHECK_LAUNCH();
    return 0;
}

int mmbert_adamw_grouped(hipStream_t stream, float* p, float* g, float* m, float* v, void* p_bf16, const uint8_t* flags,
                         const uint8_t* group_of_block, size_t n, const double* hyper, int ngroups, int step, double gscale, const float* coef,
                         int mode, int zero_grad) {
    if (n == 0) return 0;
    AdamWSlots a;
    if ((n & 255) || adamw_fill_slots(a, hyper, ngroups, step, mode) != 0) return -1;
    if (coef)
        hipLaunchKernelGGL(adamw_grouped_kernel<true>, adamw_grid(n), dim3(256), 0, stream, p, g, m, v, (bf16_t*)p_bf16, flags, group_of_block, n,
                           a, 1.0f, coef, mode, zero_grad);
    else
        hipLaunchKernelGGL(adamw_grouped_kernel<false>, adamw_grid(n), dim3(256), 0, stream, p, g, m, v, (bf16_t*)p_bf16, flags, group_of_block, n,
                           a, (float)gscale, (const float*)nullptr, mode, zero_grad);
    MMB_CHECK_LAUNCH();
    return 0;
}

// mmbert_adamw_grouped with the weight EMA fused in: the same slot table; 1 - ema_decay in double, rounded to fp32 once like the other
// coefficients.
int mmbert_adamw_ema(hipStream_t stream, float* p, float* g, float* m, float* v, void* p_bf16, const uint8_t* flags,
                     const uint8_t* group_of_block, size_t n, const double* hyper, int ngroups, int step, double gscale, const float* coef,
                     int mode, int zero_grad, float* ema, double ema_decay) {
    if (n == 0) return 0;
    AdamWSlots a;
    if ((n & 255) || adamw_fill_slots(a, hyper, ngroups, step, mode) != 0) return -1;
    if (!ema || !(ema_decay >= 0.0 && ema_decay < 1.0)) return -1;
    const float omd = (float)(1.0 - ema_decay);
    if (coef)
        hipLaunchKernelGGL(adamw_ema_kernel<true>, adamw_grid(n), dim3(256), 0, stream, p, g, m, v, ema, (bf16_t*)p_bf16, flags, group_of_block, n,
                           a, 1.0f, coef, omd, mode, zero_grad);
    else
        hipLaunchKernelGGL(adamw_ema_kernel<false>, adamw_grid(n), dim3(256), 0, stream, p, g, m, v, ema, (bf16_t*)p_bf16, flags, group_of_block, n,
                           a, (float)gscale, (const float*)nullptr, omd, mode, zero_grad);
    MMB_CHECK_LAUNCH();
    return 0;
}

// hyper as in adamw_fill_slots (the same de-duplication, the same limits) -> the LAMB coefficients of every slot, in double, rounded once
static int lamb_fill_slots(LambSlots& a, const double* hyper, int ngroups, int step) {
    return fill_slots(a, hyper, ngroups, [&](const double* h) {
        return LambCoefs{(float)h[1], (float)h[2], (float)(1.0 - h[1]), (float)(1.0 - h[2]), (float)h[3],
                         (float)(1.0 / (1.0 - pow(h[1], (double)step))), (float)(1.0 / (1.0 - pow(h[2], (double)step))), (float)h[0], (float)h[4]};
    });
}

int mmbert_lamb(hipStream_t stream, float* p, float* g, float* m, float* v, void* p_bf16, const uint8_t* flags,
                const uint8_t* group_of_block, size_t n, const double* hyper, int ngroups, int step, double gscale, const float* coef,
                int zero_grad, const int32_t* unit_of_block, const int32_t* mixed, int nmixed, const int32_t* units, int nunits,
                double max_trust, void* workspace, size_t workspace_bytes, float* ratios, float* ema, double ema_decay) {
    if (n == 0) return 0;
    LambSlots a;
    if ((n & 255) || (n >> 8) > (size_t)INT32_MAX || step < 1 || lamb_fill_slots(a, hyper, ngroups, step) != 0) return -1;
    if (!p || !g || !m || !v || !flags || !unit_of_block || !units || nunits < 1 || nmixed < 0 || (nmixed > 0 && !mixed) || !ratios) return -1;
    if (!workspace || workspace_bytes < 8 * ((n >> 8) + 4 * (size_t)nmixed) /* == MMBERT_LAMB_WORKSPACE */ || !(max_trust >= 0.0)) return -1;
    if (ema && !(ema_decay >= 0.0 && ema_decay < 1.0)) return -1;
    float2* part = (float2*)workspace;
    const int nblk = (int)(n >> 8);
    if (coef)
        hipLaunchKernelGGL(lamb_moments_kernel<true>, adamw_grid(n), dim3(256), 0, stream, p, g, m, v, flags, group_of_block, unit_of_block, mixed,
                           nmixed, n, a, 1.0f, coef, part);
    else
        hipLaunchKernelGGL(lamb_moments_kernel<false>, adamw_grid(n), dim3(256), 0, stream, p, g, m, v, flags, group_of_block, unit_of_block, mixed,
                           nmixed, n, a, (float)gscale, (const float*)nullptr, part);
    MMB_CHECK_LAUNCH();
    hipLaunchKernelGGL(lamb_fold_kernel, dim3(nunits), dim3(LAMB_FOLD_THREADS), 0, stream, (const float2*)part, flags, unit_of_block, mixed, nmixed,
                       units, nblk, (float)max_trust, ratios);
    MMB_CHECK_LAUNCH();
    if (ema)
        hipLaunchKernelGGL(lamb_apply_kernel<true>, adamw_grid(n), dim3(256), 0, stream, p, g, m, v, ema, (bf16_t*)p_bf16, flags, group_of_block,
                           unit_of_block, mixed, nmixed, ratios, nunits, n, a, (float)(1.0 - ema_decay), zero_grad);
    else
        hipLaunchKernelGGL(lamb_apply_kernel<false>, adamw_grid(n), dim3(256), 0, stream, p, g, m, v, (float*)nullptr, (bf16_t*)p_bf16, flags,
                           group_of_block, unit_of_block, mixed, nmixed, ratios, nunits, n, a, 0.f, zero_grad);
    MMB_CHECK_LAUNCH();
    return 0;
}

int mmbert_ema_swap(hipStream_t stream, float* p, float* ema, void* p_bf16, size_t n) {
    if (n == 0) return 0;
    if ((n & 255) || !p || !ema) return -1;
    hipLaunchKernelGGL(ema_swap_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, stream, p, ema, (bf16_t*)p_bf16, n);
    MMB_CHECK_LAUNCH();
    return 0;
}

static unsigned grad_norm_grid(size_t n) {
    const size_t per = (size_t)GN_THREADS * GN_UNROLL, wg = ((n + 3) / 4 + per - 1) / per;
    return (unsigned)std::max<size_t>(1, std::min<size_t>(GN_MAX_WG, wg));
}

int mmbert_grad_norm(hipStream_t stream, const float* g, size_t n, const int64_t* segs, int nseg, double norm_type, double max_norm,
                     double gscale, void* workspace, float* out) {
    const bool inf = norm_type == INFINITY;
    if ((!inf && norm_type != 2.0) || nseg < 0 || (nseg > 0 && !segs) || !workspace || !out || ((uintptr_t)g & 15) || !(max_norm >= 0.0))
        return -1;
    const unsigned grid = grad_norm_grid(n);
    double* part = (double*)workspace;
    if (inf) hipLaunchKernelGGL(grad_norm_partial_kernel<true>, dim3(grid), dim3(GN_THREADS), 0, stream, g, n, (const long long*)segs, nseg, part);
    else hipLaunchKernelGGL(grad_norm_partial_kernel<false>, dim3(grid), dim3(GN_THREADS), 0, stream, g, n, (const long long*)segs, nseg, part);
    MMB_CHECK_LAUNCH();
    if (inf) hipLaunchKernelGGL(grad_norm_finalize_kernel<true>, dim3(1), dim3(GN_THREADS), 0, stream, (const double*)part, (int)grid, (float)max_norm, gscale, out);
    else hipLaunchKernelGGL(grad_norm_finalize_kernel<false>, dim3(1), dim3(GN_THREADS), 0, stream, (const double*)part, (int)grid, (float)max_norm, gscale, out);
    MMB_CHECK_LAUNCH();
    return 0;
}

int mmbert_grad_scale(hipStream_t stream, float* g, size_t n, const int64_t* segs, int nseg, const float* coef) {
    if (nseg < 0 || (nseg > 0 && !segs) || !coef || ((uintptr_t)g & 15)) return -1;
    if (nseg == 0 || n == 0) return 0;
    hipLaunchKernelGGL(grad_scale_kernel, dim3(grad_norm_grid(n)), dim3(GN_THREADS), 0, stream, g, n, (const long long*)segs, nseg, coef);
    MMB_CHECK_LAUNCH();
    return 0;
}

int mmbert_gelu_bwd(hipStream_t stream, const void* dy, const void* u, void* du, size_t n) {
    if (n == 0) return 0;
    if (n & 3) return -1;
    hipLaunchKernelGGL(gelu_bwd_kernel, dim3(grid_for(n / 4, 256, 4096)), dim3(256), 0, stream, (const bf16_t*)dy, (const bf16_t*)u, (bf16_t*)du, n);
    MMB_CHECK_LAUNCH();
    return 0;
}

int mmbert_cast_f32_bf16(hipStream_t stream, const float* x, void* y, size_t n) {
    if (n == 0) return 0;
    if (n & 3) return -1;
    hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3(grid_for(n / 4, 256, 4096)), dim3(256), 0, stream, x, (bf16_t*)y, n);
    MMB_CHECK_LAUNCH();
    return 0;
}

int mmbert_cast_bf16_f32(hipStream_t stream, const void* x, float* y, size_t n) {
    if (n == 0) return 0;
    if (n & 3) return -1;
    hipLaunchKernelGGL(cast_bf16_f32_kernel, dim3(grid_for(n / 4, 256, 4096)), dim3(256), 0, stream, (const bf16_t*)x, y, n);
    MMB_CHECK_LAUNCH();
    return 0;
}

// descs: device array of {src_off, dst_off, rows, cols, dst_ld, tile0}; total_tiles = sum of 64x64 tiles
int mmbert_transpose_cast(hipStream_t stream, const float* src, void* dst, const void* descs, int ndesc, int total_tiles) {
    if (ndesc <= 0 || total_tiles <= 0) return 0;
    hipLaunchKernelGGL(transpose_cast_kernel<float>, dim3(total_tiles), dim3(256), 0, stream, src, (bf16_t*)dst, (const TransDesc*)descs, ndesc);
    MMB_CHECK_LAUNCH();
    return 0;
}

// the same from a bf16 source laid out like the fp32 one (same element offsets)
int mmbert_transpose_bf16(hipStream_t stream, const void* src, void* dst, const void* descs, int ndesc, int total_tiles) {
    if (ndesc <= 0 || total_tiles <= 0) return 0;
    hipLaunchKernelGGL(transpose_cast_kernel<bf16_t>, dim3(total_tiles), dim3(256), 0, stream, (const bf16_t*)src, (bf16_t*)dst, (const TransDesc*)descs, ndesc);
    MMB_CHECK_LAUNCH();
    return 0;
}

// out[i] = map[ i < n ? rows[i] : extra[i - n] ]  as int64 AND int32 (map optional): the row list of the top encoder layer's sparse
// backward -- labelled rows, then the [CLS] rows, in the encoder's packed order -- in one launch (round 3: an int32->int64 cast, a cat,
// an index_select through the packing's inverse map and an int64->int32 cast)
// (inv_stamp, optional: the INVERSE of the list for mmbert_scatter_rows_zero -- inv_stamp[out[i]] = stamp << 32 | i in a persistent
// int64 array over all rows that is never cleared: an entry counts only while its upper half equals the current call's stamp)
__global__ void compact_rows_kernel(const int* __restrict__ a32, const int64_t* __restrict__ a64, int n, const int64_t* __restrict__ extra, int nextra,
                                    const int64_t* __restrict__ map, int64_t* __restrict__ out64, int* __restrict__ out32,
                                    long long* __restrict__ inv_stamp, long long stamp_hi) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n + nextra) return;
    int64_t r = i < n ? (a32 ? (int64_t)a32[i] : a64[i]) : extra[i - n];
    if (map) r = map[r];
    out64[i] = r;
    out32[i] = (int)r;
    if (inv_stamp) inv_stamp[r] = stamp_hi | (long long)i;
}
static int compact_rows_launch(hipStream_t stream, const int* rows32, const int64_t* rows64, int n, const int64_t* extra, int nextra, const int64_t* map,
                               int64_t* out64, int* out32, long long* inv_stamp, unsigned stamp) {
    if (n < 0 || nextra < 0 || (n > 0 && !rows32 && !rows64) || (nextra > 0 && !extra)) return -1;
    if (n + nextra == 0) return 0;
    hipLaunchKernelGGL(compact_rows_kernel, dim3((n + nextra + 255) / 256), dim3(256), 0, stream, rows32, rows64, n, extra, nextra, map, out64, out32,
                       inv_stamp, (long long)((unsigned long long)stamp << 32));
    MMB_CHECK_LAUNCH();
    return 0;
}
int mmbert_compact_rows(hipStream_t stream, const int* rows32, const int64_t* rows64, int n, const int64_t* extra, int nextra, const int64_t* map,
                        int64_t* out64, int* out32) {
    return compact_rows_launch(stream, rows32, rows64, n, extra, nextra, map, out64, out32, nullptr, 0u);
}
int mmbert_compact_rows_inv(hipStream_t stream, const int* rows32, const int64_t* rows64, int n, const int64_t* extra, int nextra, const int64_t* map,
                            int64_t* out64, int* out32, int64_t* inv_stamp, unsigned stamp) {
    if (!inv_stamp || stamp == 0u) return -1;
    return compact_rows_launch(stream, rows32, rows64, n, extra, nextra, map, out64, out32, (long long*)inv_stamp, stamp);
}

// dst_k[r] = src_k[i] where the stamped inverse says row r is entry i of the current list, ZERO otherwise, for r < nrows and up to 4
// matrices k: a zero fill and an index_copy_ per matrix in one launch (the sparse top layer's gradients going back to full height).
struct ScatterSeg { const char* src; char* dst; long long src_pitch, dst_pitch; int row_bytes; };
struct ScatterArgs { ScatterSeg s[4]; };
__global__ __launch_bounds__(256) void scatter_rows_zero_kernel(const ScatterArgs a, const long long* __restrict__ inv_stamp, long long stamp_hi, int nlist) {
    const ScatterSeg s = a.s[blockIdx.y];
    const int r = blockIdx.x;
    const long long v = inv_stamp[r];
    const int i = (int)(v & 0xffffffffll);
    const bool hit = (v & ~0xffffffffll) == stamp_hi && i < nlist;
    char* dst = s.dst + (long long)r * s.dst_pitch;
    const char* src = s.src + (long long)(hit ? i : 0) * s.src_pitch;
    for (int b = threadIdx.x * 16; b < s.row_bytes; b += 256 * 16) {
        uint4 x = {0u, 0u, 0u, 0u};
        if (hit) x = *(const uint4*)(src + b);
        *(uint4*)(dst + b) = x;
    }
}
int mmbert_scatter_rows_zero(hipStream_t stream, int nseg, const void* const* src, void* const* dst, const long long* src_pitch, const long long* dst_pitch,
                             const int* row_bytes, const int64_t* inv_stamp, unsigned stamp, int nlist, int nrows) {
    if (nseg <= 0 || nrows <= 0) return 0;
    if (nseg > 4 || !inv_stamp || stamp == 0u || nlist < 0) return -1;
    ScatterArgs a = {};
    for (int k = 0; k < nseg; ++k) {
        if (!dst[k] || (nlist > 0 && !src[k]) || row_bytes[k] <= 0 || ((row_bytes[k] | src_pitch[k] | dst_pitch[k]) & 15) ||
            (((uintptr_t)src[k] | (uintptr_t)dst[k]) & 15)) return -1;
        a.s[k].src = (const char*)src[k]; a.s[k].dst = (char*)dst[k]; a.s[k].src_pitch = src_pitch[k]; a.s[k].dst_pitch = dst_pitch[k];
        a.s[k].row_bytes = row_bytes[k];
    }
    hipLaunchKernelGGL(scatter_rows_zero_kernel, dim3(nrows, nseg), dim3(256), 0, stream, a, (const long long*)inv_stamp,
                       (long long)((unsigned long long)stamp << 32), nlist);
    MMB_CHECK_LAUNCH();
    return 0;
}

int mmbert_gather_rows(hipStream_t stream, int nseg, const void* const* src, void* const* dst, const long long* src_pitch, const long long* dst_pitch,
                       const int* row_bytes, const int* idx, int nrows) {
    if (nseg <= 0 || nrows <= 0) return 0;
    if (nseg > 12) return -1;
    GatherArgs a = {};
    for (int k = 0; k < nseg; ++k) {
        if (!src[k] || !dst[k] || row_bytes[k] <= 0 || (row_bytes[k] & 3) || (src_pitch[k] & 3) || (dst_pitch[k] & 3) ||
            ((uintptr_t)src[k] & 3) || ((uintptr_t)dst[k] & 3)) return -1;
        a.s[k].src = (const char*)src[k]; a.s[k].dst = (char*)dst[k]; a.s[k].src_pitch = src_pitch[k]; a.s[k].dst_pitch = dst_pitch[k];
        a.s[k].row_bytes = row_bytes[k];
        a.s[k].vec16 = !((row_bytes[k] | src_pitch[k] | dst_pitch[k]) & 15) && !(((uintptr_t)src[k] | (uintptr_t)dst[k]) & 15);
    }
    hipLaunchKernelGGL(gather_rows_kernel, dim3(nrows, nseg), dim3(256), 0, stream, a, idx);
    MMB_CHECK_LAUNCH();
    return 0;
}

int mmbert_rows_to_block(hipStream_t stream, const int64_t* ids, const void* rows, int rows_bf16, int ldr, int n, int H,
                         const int64_t* uni, int U, int V, float* block) {
    if (n <= 0 || U <= 0) return 0;
    if (!ids || !rows || !uni || !block || H <= 0 || ldr < H) return -1;
    hipLaunchKernelGGL(rows_to_block_kernel, dim3(n), dim3(256), 0, stream, ids, rows, rows_bf16, ldr, n, H, uni, U, V, block);
    MMB_CHECK_LAUNCH();
    return 0;
}

int mmbert_pack_i64(hipStream_t stream, int nseg, const int64_t* const* src, const long long* dst_offset, const long long* count,
                    const long long* fill, int64_t* out) {
    if (nseg <= 0) return 0;
    if (nseg > 12 || !out) return -1;
    PackArgs a = {};
    long long most = 0;
    for (int k = 0; k < nseg; ++k) {
        if (count[k] < 0 || dst_offset[k] < 0) return -1;
        a.s[k].src = src[k]; a.s[k].dst0 = dst_offset[k]; a.s[k].n = count[k]; a.s[k].fill = fill[k];
        most = count[k] > most ? count[k] : most;
    }
    if (most == 0) return 0;
    hipLaunchKernelGGL(pack_i64_kernel, dim3(grid_for((size_t)most, 256, 256), nseg), dim3(256), 0, stream, a, out);
    MMB_CHECK_LAUNCH();
    return 0;
}

int mmbert_mlm_mask(hipStream_t stream, int64_t* ids, int64_t* labels, size_t n, uint32_t rng_stream, uint32_t select_thr16,
                    uint32_t replace_thr16, int64_t special0, int64_t special1, int64_t special2, int64_t mask_id) {
    if (n == 0) return 0;
    if (n >= ((size_t)1 << 32) || select_thr16 > 65536u || replace_thr16 > 65536u) return -1;
    hipLaunchKernelGGL(mlm_mask_kernel, dim3(grid_for(n, 256, 1024)), dim3(256), 0, stream, ids, labels, n, rng_stream, select_thr16,
                       replace_thr16, special0, special1, special2, mask_id);
    MMB_CHECK_LAUNCH();
    return 0;
}

int mmbert_dropout_mask(hipStream_t stream, uint8_t* out, size_t n, uint32_t rng_stream, uint32_t thr16) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(dropout_mask_kernel, dim3(grid_for(n, 256, 4096)), dim3(256), 0, stream, out, n, rng_stream, thr16);
    MMB_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
