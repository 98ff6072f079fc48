// duo_decode_multi.hip — a decode step of 2..64 query tokens over the bf16 static pools (gfx950).
//
// The reference runs such a step (llama.py:374-421 with q_len = T: a speculative-decoding verify step, a short chat turn,
// the ragged tail of a chunked prefill) through the same two flash_attn_func calls as a prefill chunk.  The prefill kernel
// gives a workgroup to (256 query rows x one q head) and walks a kv head's rows once per q head of its group; at T = 4 it
// fills 4 of 64 query rows.  This kernel is the split-KV stream of the single-token scan (duo_decode.hip) with both products
// on v_mfma_f32_16x16x32_bf16, laid out as duo_int4_decode_mfma_kernel<_, true> (duo_int4.hip) minus the dequantisation:
//
//   * a 256-thread workgroup per (kv head, split, column block); each of its four waves streams a quarter of the split's keys
//     in 32-key tiles and the four partial states are combined through LDS;
//   * the 16 q columns of the fragments carry tpb = 16 / group tokens: column c = (token tok0 + c / group, q head
//     qh0 + c % group), tok0 = blockIdx.y * tpb — one pass over the kv head's rows serves tpb tokens of the whole GQA group;
//   * S^T[32 keys x 16 cols] = K . Q^T: K rows go from HBM straight into the A operand (lane (r, g) holds dims 32 kb + 8 g .. + 7
//     of key r), 16 B per lane, non-temporal, the next tile's 16 loads issued before the current tile is touched;
//   * V rows (16 lanes per 256-B row) go through a wave-private 8 KiB LDS tile and come back transposed (ds_read_b64_tr_b16)
//     as the B operand of O += P . V;
//   * softmax in fp32 in the exp2 domain against a per-column reference maximum that is raised (and O rescaled) only when a
//     score exceeds it by more than 2^8; P is rounded to bf16 before P . V, its row sums are taken before the rounding (the
//     prefill kernel's arithmetic, FA2's);
//   * keys: segment A entirely, segment B (the step's T rows) causally — column token i sees segB row j iff j <= i.  A tile
//     wholly inside segment A runs the unmasked body with uniform row bases; the (at most ceil(T / 32) + 1) tiles that touch
//     segment B, and the partial last tile of a wave's range, run the general body: row source chosen per row, row index
//     clamped to the wave's last live row, element mask by SELECTION (a masked probability is the constant 0).  A column that
//     sees nothing in a wave's range leaves m = sentinel, l = 0, O = 0 and weighs 0 in the combine and in the merge;
//   * partials (m, l, O[128]) per (token, q head, split) in an fp32 workspace, merged by duo_decode_multi_merge_kernel —
//     no atomics anywhere: repeated runs are bit-equal.
#include <algorithm>
#include <type_traits>
#include "duo_common.h"
#include "duo_decode_plan.h"

namespace {

constexpr float kNegSentinelM = -1.0e30f;

struct MultiParams {
    const bf16_t *q;
    bf16_t *out;
    int64_t q_ts, q_hs, q_bs;         // q elements between tokens / q heads / batch rows
    int64_t out_ts, out_hs, out_bs;
    DuoClassDev cls[2];               // 0 = retrieval (full), 1 = streaming; b.len == n_tokens
    int32_t splits[2];
    int32_t nblk_full;                // cls[0].n_kv_heads * splits[0]
    int32_t group, n_tokens, tpb;
    float scale_log2e;
    float *ws_ml, *ws_acc;            // per (batch row, token): [n_q_heads][max_splits][2] then [n_q_heads][max_splits][128]
    int32_t max_splits;
    int64_t ws_row_floats;            // floats between the partial areas of two (batch row, token) pairs
};

typedef __attribute__((address_space(1))) const uint8_t gbyte_t;
typedef __attribute__((address_space(1))) const u32x4 gu32x4_t;
typedef __attribute__((address_space(3))) u32x4 lds_u32x4;

// a uniform address as an SGPR pair in the global address space: the loads then take the sgpr-base + vgpr32-offset form
__device__ __forceinline__ gbyte_t *ubase(const uint8_t *p) {
    const uint64_t a = (uint64_t)p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    return (gbyte_t *)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ u32x4 ld16_nt(gbyte_t *p) { return __builtin_nontemporal_load(reinterpret_cast<gu32x4_t *>(p)); }
__device__ __forceinline__ u32x4 ld16_nt(const uint8_t *p) { return __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p)); }
__device__ __forceinline__ bf16x8 as_frag(const u32x4 &w) { return *reinterpret_cast<const bf16x8 *>(&w); }

typedef __attribute__((ext_vector_type(2))) __bf16 hw_bf16x2_m;
typedef __attribute__((ext_vector_type(2))) float f32x2_m;
__device__ __forceinline__ uint32_t cvt_pk_bf16_m(float lo, float hi) {
    f32x2_m v = {lo, hi};
    hw_bf16x2_m r = __builtin_convertvector(v, hw_bf16x2_m);   // v_cvt_pk_bf16_f32: round to nearest even
    return *reinterpret_cast<uint32_t *>(&r);
}

// One 32-key tile in registers.  k[4 h + kb]: key 16 h + r, dims 32 kb + 8 g .. + 7 (the A operand of k-step kb);
// v[i]: key 4 i + g, dims 8 r .. + 7 (a wave-load covers four whole 256-B rows).
struct MTile {
    u32x4 k[8], v[8];
};

// The wave's 8 KiB V tile, [32 keys][16 chunks of 16 B], chunk c of key k stored at slot c ^ (k & 15) (the layout of
// duo_int4.hip's V^ tile).  Transpose read: lane i of a 16-lane group supplies the 8-byte piece (row i >> 2, cols 4 (i & 3) .. + 3)
// of a 4 x 16 block and receives column i; rows 4 g .. 4 g + 3 (and + 16 at + 4096), dim block nb at address ^ (nb << 5).
// Every address is a multiple of 8 and inside the tile, and the reads run with all 64 lanes active.
__device__ __forceinline__ uint32_t mt_lds_wa(uint32_t lbase, int key, int chunk) {
    return lbase + key * 256 + ((chunk ^ (key & 15)) << 4);
}
__device__ __forceinline__ uint32_t mt_lds_ra(uint32_t lbase, int r, int g) {
    const int kr = 4 * g + (r >> 2);
    return lbase + kr * 256 + ((((r >> 1) & 1) ^ (kr & 15)) << 4) + 8 * (r & 1);
}

// O += P . V from the wave's LDS tile: transpose reads two dim blocks at a time, one batch ahead of the MFMAs, with counted
// lgkmcnt waits.  (Macros, not loops over functions: ds_read_b64_tr_b16 takes its offset as an immediate.)  O[nb][e] is
// (q column 4 g + e, dim 16 nb + r); k-slot 4 h + e of lane group g is key 16 h + 4 g + e on both operands.
__device__ __forceinline__ void mt_pv(const bf16x8 &pA, uint32_t ra, f32x4 (&O)[8]) {
    u32x2 va[4], vb[4];
    __builtin_amdgcn_sched_barrier(0);
#define DUO_MT_TR_READ(dst, addr, off) \
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off) : "memory")
#define DUO_MT_TR_BATCH(buf, nb0)                                                   \
    _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) {                              \
        uint32_t a_ = ra ^ (uint32_t)(((nb0) + i_) << 5);                           \
        DUO_MT_TR_READ(buf[2 * i_], a_, 0);                                         \
        DUO_MT_TR_READ(buf[2 * i_ + 1], a_, 4096);                                  \
    }
#define DUO_MT_PV(buf, nb0)                                                                               \
    _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) {                                                    \
        const u32x4 w_ = {buf[2 * i_].x, buf[2 * i_].y, buf[2 * i_ + 1].x, buf[2 * i_ + 1].y};            \
        O[(nb0) + i_] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pA, as_frag(w_), O[(nb0) + i_], 0, 0, 0); \
    }
#define DUO_MT_WAIT(n) do { asm volatile("s_waitcnt lgkmcnt(" #n ")" ::: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)
    DUO_MT_TR_BATCH(va, 0);
    DUO_MT_TR_BATCH(vb, 2);
    DUO_MT_WAIT(4);
    DUO_MT_PV(va, 0);
    __builtin_amdgcn_sched_barrier(0);
    DUO_MT_TR_BATCH(va, 4);
    DUO_MT_WAIT(4);
    DUO_MT_PV(vb, 2);
    __builtin_amdgcn_sched_barrier(0);
    DUO_MT_TR_BATCH(vb, 6);
    DUO_MT_WAIT(4);
    DUO_MT_PV(va, 4);
    DUO_MT_WAIT(0);
    DUO_MT_PV(vb, 6);
#undef DUO_MT_TR_READ
#undef DUO_MT_TR_BATCH
#undef DUO_MT_PV
#undef DUO_MT_WAIT
}

__global__ __launch_bounds__(256, 2) void duo_decode_multi_kernel(const MultiParams P) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15;    // key row inside a 16-key half / q column / dim column
    const int g = lane >> 4;    // k-slot group

    // block -> head class, kv head, split; the split's balanced share of the 64-key units; a quarter of it (whole 32-key
    // tiles) per wave
    int b = blockIdx.x;
    const bool ci = b >= P.nblk_full;
    if (ci) b -= P.nblk_full;
    const DuoClassDev C = duo_select(P.cls[0], P.cls[1], ci);
    const int splits = ci ? P.splits[1] : P.splits[0];
    const int kvh = b / splits, split = b - kvh * splits;
    const int qh0 = C.q_head_offset + kvh * P.group;
    const int lenA = C.a.len, L = lenA + C.b.len;
    int w0, w1;
    {
        const int units = (L + 63) >> 6;
        const int uq = units / splits, ur = units - uq * splits;
        const int u0 = split * uq + min(split, ur);
        const int un = uq + (split < ur ? 1 : 0);
        const int c0 = u0 << 6;
        const int c1 = min((u0 + un) << 6, L);
        const int per_wave = (((c1 - c0 + 3) >> 2) + 31) & ~31;
        w0 = __builtin_amdgcn_readfirstlane(c0 + wave * per_wave);
        w1 = __builtin_amdgcn_readfirstlane(min(w0 + per_wave, c1));
    }
    // row 0 of the kv head in either segment (grid.z = batch row), strides in bytes
    const int64_t tsA = C.a.token_stride * 2, tsB = C.b.token_stride * 2;
    const uint8_t *kA = reinterpret_cast<const uint8_t *>(C.a.k + (int64_t)kvh * C.a.head_stride + (int64_t)blockIdx.z * C.a.batch_stride);
    const uint8_t *vA = reinterpret_cast<const uint8_t *>(C.a.v + (int64_t)kvh * C.a.head_stride + (int64_t)blockIdx.z * C.a.batch_stride);
    const uint8_t *kB = reinterpret_cast<const uint8_t *>(C.b.k + (int64_t)kvh * C.b.head_stride + (int64_t)blockIdx.z * C.b.batch_stride);
    const uint8_t *vB = reinterpret_cast<const uint8_t *>(C.b.v + (int64_t)kvh * C.b.head_stride + (int64_t)blockIdx.z * C.b.batch_stride);

    // this lane's column: its token and q head, whether it is a column of the step at all, and the last key it sees inside
    // this wave's range.  Padding columns load zeros, see nothing and never vote; their reference stays 0 so that the
    // probabilities of their (all-zero) scores stay finite in the unmasked body.
    const int tok0 = blockIdx.y * P.tpb;
    const int tl = r / P.group, tok = tok0 + tl;
    const bool col = tok < P.n_tokens;
    const int lim_w = col ? min(w1 - 1, lenA + tok) : -1;

    // Q^T fragments: column r, dims 32 kb + 8 g .. + 7
    bf16x8 qB[4];
    {
        const bf16_t *qcol = P.q + (int64_t)blockIdx.z * P.q_bs + (int64_t)tok * P.q_ts + (int64_t)(qh0 + r - tl * P.group) * P.q_hs;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            u32x4 w = {0u, 0u, 0u, 0u};
            if (col) w = *reinterpret_cast<const u32x4 *>(qcol + 32 * kb + 8 * g);
            qB[kb] = as_frag(w);
        }
    }

    __shared__ __attribute__((aligned(16))) uint8_t lds[4 * 8192];
    const uint32_t lbase = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const uint8_t *)lds + wave * 8192;
    uint32_t wa[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) wa[i] = mt_lds_wa(lbase, 4 * i + g, r);
    const uint32_t ra = mt_lds_ra(lbase, r, g);

    f32x4 O[8];
#pragma unroll
    for (int nb = 0; nb < 8; ++nb) O[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_ref = col ? kNegSentinelM : 0.f;    // per q column, log2 domain (scores x scale x log2 e)
    float lsum = 0.f;                           // this lane's share (its 8 keys of every tile) of the column's row sum
    const float c_ = P.scale_log2e;

    // A tile wholly inside segment A: uniform row bases (SGPR pairs) + two constant per-lane offsets.  (The empty asm
    // re-materialises the 32-bit offsets in the basic block of the loads so that they select the sgpr-base + vgpr32-offset
    // addressing form.)
    uint32_t ko = (uint32_t)r * (uint32_t)tsA + 16u * g, vo = (uint32_t)g * (uint32_t)tsA + 16u * r;
    auto load_full = [&](int t, MTile &T) __attribute__((always_inline)) {
        const uint8_t *kt = kA + (int64_t)t * tsA, *vt = vA + (int64_t)t * tsA;
        asm volatile("" : "+v"(ko), "+v"(vo));
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            gbyte_t *kh = ubase(kt + 16 * h * tsA);
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) T.k[4 * h + kb] = ld16_nt(kh + ko + 64 * kb);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) T.v[i] = ld16_nt(ubase(vt + 4 * i * tsA) + vo);
    };
    // Any other tile: the row source (base and stride of A or B) chosen per row; a row index past the wave's range re-reads
    // the range's last row (live by construction: w1 <= L) and is masked later.
    auto load_general = [&](int t, MTile &T) __attribute__((always_inline)) {
        const int last = w1 - 1;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int row = min(t + 16 * h + r, last);
            const bool inA = row < lenA;
            const uint8_t *p = (inA ? kA + (int64_t)row * tsA : kB + (int64_t)(row - lenA) * tsB) + 16 * g;
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) T.k[4 * h + kb] = ld16_nt(p + 64 * kb);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int row = min(t + 4 * i + g, last);
            const bool inA = row < lenA;
            const uint8_t *p = (inA ? vA + (int64_t)row * tsA : vB + (int64_t)(row - lenA) * tsB) + 16 * r;
            T.v[i] = ld16_nt(p);
        }
    };

    // One tile.  MASKED: keys past the wave's range or past the column's causal limit are masked by selection.
    auto process = [&](const MTile &T, int t, auto masked_tag) __attribute__((always_inline)) {
        constexpr bool MASKED = decltype(masked_tag)::value;
        // ---- S^T = K . Q^T ---------------------------------------------------------------------------
        f32x4 S[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            S[h] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
                S[h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(T.k[4 * h + kb]), qB[kb], S[h], 0, 0, 0);
        }
        // ---- V -> LDS (issued early: the writes drain while the softmax runs) --------------------------
#pragma unroll
        for (int i = 0; i < 8; ++i) *(lds_u32x4 *)(uintptr_t)wa[i] = T.v[i];
        // ---- softmax against the reference maximum: S[h][e] is (key t + 16 h + 4 g + e, column r) ------
        float sv[8];
        bool vis[8];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                sv[4 * h + e] = S[h][e] * c_;
                vis[4 * h + e] = !MASKED || t + 16 * h + 4 * g + e <= lim_w;
            }
        float mx;
        if constexpr (MASKED) {
            // a column without a visible key votes with the sentinel itself and so neither triggers the raise nor moves
            float sm[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) sm[i] = vis[i] ? sv[i] : kNegSentinelM;
            mx = fmaxf(fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3])), fmaxf(fmaxf(sm[4], sm[5]), fmaxf(sm[6], sm[7])));
        } else {
            mx = fmaxf(fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3])), fmaxf(fmaxf(sv[4], sv[5]), fmaxf(sv[6], sv[7])));
            mx = col ? mx : kNegSentinelM;
        }
        if (__any(mx > m_ref + 8.f)) {
            // raise the reference to the running maximum of every q column and rescale: lsum is this lane's own column's,
            // O's rows are q columns 4 g + e, whose factors come from the lanes that own those columns
            float tm = fmaxf(mx, __shfl_xor(mx, 16));
            tm = fmaxf(tm, __shfl_xor(tm, 32));
            const float m_new = fmaxf(m_ref, tm);
            const float alpha = fast_exp2(m_ref - m_new);
            m_ref = m_new;
            lsum *= alpha;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float a = __shfl(alpha, 4 * g + e);
#pragma unroll
                for (int nb = 0; nb < 8; ++nb) O[nb][e] *= a;
            }
        }
        float p[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            p[i] = fast_exp2(sv[i] - m_ref);
            if constexpr (MASKED) p[i] = vis[i] ? p[i] : 0.f;
        }
        lsum += ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
        u32x4 pw;
        pw.x = cvt_pk_bf16_m(p[0], p[1]);
        pw.y = cvt_pk_bf16_m(p[2], p[3]);
        pw.z = cvt_pk_bf16_m(p[4], p[5]);
        pw.w = cvt_pk_bf16_m(p[6], p[7]);
        // ---- O += P . V ----------------------------------------------------------------------------------
        mt_pv(as_frag(pw), ra, O);
    };

    // Main loop over the tiles wholly inside segment A: straight-line code with a fixed number of loads in flight (the next
    // tile's 16 loads are issued, unconditionally, before the current tile is touched; after the last such tile the prefetch
    // re-reads it).  The tiles behind them — those that touch segment B and the partial last one — take the general body.
    const int wE = w0 + ((max(min(w1, lenA) - w0, 0) >> 5) << 5);
    if (w0 < wE) {
        const int t_last = wE - 32;
        int t = w0;
        MTile A, B;
        load_full(t, A);
        for (;;) {
            load_full(min(t + 32, t_last), B);
            __builtin_amdgcn_sched_barrier(0);
            process(A, t, std::false_type{});
            t += 32;
            if (t > t_last) break;
            load_full(min(t + 32, t_last), A);
            __builtin_amdgcn_sched_barrier(0);
            process(B, t, std::false_type{});
            t += 32;
            if (t > t_last) break;
        }
    }
    for (int t = max(wE, w0); t < w1; t += 32) {
        MTile X;
        load_general(t, X);
        process(X, t, std::true_type{});
    }

    // the column's row sum: the four k-slot groups hold disjoint keys
    lsum += __shfl_xor(lsum, 16);
    lsum += __shfl_xor(lsum, 32);

    // ---- combine the 4 waves through LDS ------------------------------------------------------
    __syncthreads();   // every wave is done with its V tile: the LDS is reused for the partials
    float *s_acc = reinterpret_cast<float *>(lds);                 // [4 waves][16 q][128 dims]  = 32 KiB
    __shared__ float s_ml[4][16][2];
    if (g == 0) {
        s_ml[wave][r][0] = m_ref;
        s_ml[wave][r][1] = lsum;
    }
#pragma unroll
    for (int nb = 0; nb < 8; ++nb)
#pragma unroll
        for (int e = 0; e < 4; ++e) s_acc[(wave * 16 + 4 * g + e) * DUO_HEAD_DIM + 16 * nb + r] = O[nb][e];
    __syncthreads();
    const int n_cols = min(P.tpb, P.n_tokens - tok0) * P.group;      // the step's columns in this block
    for (int idx = threadIdx.x; idx < n_cols * DUO_HEAD_DIM; idx += 256) {
        const int q = idx >> 7;
        const int d = idx & 127;
        float M = s_ml[0][q][0];
#pragma unroll
        for (int w = 1; w < 4; ++w) M = fmaxf(M, s_ml[w][q][0]);
        float Lsum = 0.f, o = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float sc = fast_exp2(s_ml[w][q][0] - M);
            Lsum = fmaf(s_ml[w][q][1], sc, Lsum);
            o = fmaf(s_acc[(w * 16 + q) * DUO_HEAD_DIM + d], sc, o);
        }
        const int qtl = q / P.group, qtok = tok0 + qtl;
        const int qh = qh0 + q - qtl * P.group;
        if (splits == 1) {
            P.out[(int64_t)blockIdx.z * P.out_bs + (int64_t)qtok * P.out_ts + (int64_t)qh * P.out_hs + d] = (bf16_t)f32_to_bf16_bits(o / Lsum);
        } else {
            const int64_t ws_row = ((int64_t)blockIdx.z * P.n_tokens + qtok) * P.ws_row_floats;
            const int64_t slot = (int64_t)qh * P.max_splits + split;
            P.ws_acc[ws_row + slot * DUO_HEAD_DIM + d] = o;
            if (d == 0) {
                P.ws_ml[ws_row + slot * 2 + 0] = M;
                P.ws_ml[ws_row + slot * 2 + 1] = Lsum;
            }
        }
    }
}

struct MultiMergeParams {
    const float *ws_ml, *ws_acc;
    bf16_t *out;
    int64_t out_ts, out_hs, out_bs;
    int32_t max_splits, n_tokens;
    int32_t qh_begin[2], qh_end[2], splits[2];
    int64_t ws_row_floats;
};

// Merge of the split-KV partials: grid = (q heads with more than one split, 4 dim quarters, batch rows x tokens).  The form of
// duo_decode_merge_task (duo_decode.hip): 8 threads x 4 dims across, 32 split lanes deep, every split lane folds its own
// splits against its own running maximum, the 32 lanes are combined through LDS with their maxima.
__global__ __launch_bounds__(256) void duo_decode_multi_merge_kernel(const MultiMergeParams P) {
    int qh = blockIdx.x, splits;
    {
        const int n0 = P.splits[0] > 1 ? P.qh_end[0] - P.qh_begin[0] : 0;
        if (qh < n0) { qh += P.qh_begin[0]; splits = P.splits[0]; }
        else { qh = qh - n0 + P.qh_begin[1]; splits = P.splits[1]; }
    }
    const int row = blockIdx.z, brow = row / P.n_tokens, tok = row - brow * P.n_tokens;
    const int sl = threadIdx.x >> 3, dq = threadIdx.x & 7;
    const int d0 = blockIdx.y * 32 + dq * 4;
    const float *ml = P.ws_ml + (int64_t)row * P.ws_row_floats + (int64_t)qh * P.max_splits * 2;
    const float *ac = P.ws_acc + (int64_t)row * P.ws_row_floats + (int64_t)qh * P.max_splits * DUO_HEAD_DIM + d0;
    __shared__ float sm[32];
    __shared__ float slm[32][8];
    __shared__ f32x4 so[32][8];
    float m = kNegSentinelM, Lsum = 0.f;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    for (int s = sl; s < splits; s += 128) {
        float wm[4], wl[4];
        f32x4 a[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            ok[u] = s + 32 * u < splits;
            const int si = ok[u] ? s + 32 * u : s;
            wm[u] = ml[si * 2];
            wl[u] = ml[si * 2 + 1];
            a[u] = *reinterpret_cast<const f32x4 *>(ac + (int64_t)si * DUO_HEAD_DIM);
        }
        float mx = m;
#pragma unroll
        for (int u = 0; u < 4; ++u) mx = fmaxf(mx, ok[u] ? wm[u] : kNegSentinelM);
        const float f = fast_exp2(m - mx);
        Lsum *= f;
        o = o * f;
        m = mx;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float wu = ok[u] ? fast_exp2(wm[u] - m) : 0.f;
            Lsum = fmaf(wl[u], wu, Lsum);
            o = o + a[u] * wu;
        }
    }
    if (dq == 0) sm[sl] = m;
    slm[sl][dq] = Lsum;
    so[sl][dq] = o;
    __syncthreads();
    if (sl == 0) {
        float M = sm[0];
#pragma unroll
        for (int i = 1; i < 32; ++i) M = fmaxf(M, sm[i]);
        float LL = 0.f;
        f32x4 oo = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const float f = fast_exp2(sm[i] - M);      // lanes without a split: exp2(-huge) = 0
            LL = fmaf(slm[i][dq], f, LL);
            oo = oo + so[i][dq] * f;
        }
        const float inv = 1.f / LL;
        u32x2 w;
        w.x = pack_bf16x2(oo.x * inv, oo.y * inv);
        w.y = pack_bf16x2(oo.z * inv, oo.w * inv);
        *reinterpret_cast<u32x2 *>(P.out + (int64_t)brow * P.out_bs + (int64_t)tok * P.out_ts + (int64_t)qh * P.out_hs + d0) = w;
    }
}

}  // namespace

extern "C" int64_t duo_attn_decode_multi_workspace_bytes(int32_t n_q_heads, int32_t n_tokens, int32_t max_splits) {
    if (n_q_heads <= 0 || n_tokens <= 0 || max_splits <= 0) return 0;
    return (int64_t)n_tokens * n_q_heads * max_splits * (DUO_HEAD_DIM + 2) * (int64_t)sizeof(float);
}

extern "C" int duo_attn_decode_multi_batched_bf16(const void *q, int64_t q_batch_stride, int64_t q_token_stride,
                                                  int64_t q_head_stride, void *out, int64_t out_batch_stride,
                                                  int64_t out_token_stride, int64_t out_head_stride, int32_t n_batch,
                                                  int32_t n_tokens, int32_t group, const duo_head_class *full,
                                                  const duo_head_class *stream_cls, float scale, int32_t head_dim,
                                                  void *workspace, int64_t workspace_bytes, void *stream) {
    if (head_dim != DUO_HEAD_DIM) return DUO_EHEADDIM;
    if (!q || !out || group <= 0 || n_batch < 0 || n_tokens < 1 || n_tokens > 64 || (int64_t)n_batch * n_tokens > 65535)
        return DUO_EINVAL;
    if (n_tokens == 1)      // the single-token scan (any group it supports), bit for bit
        return duo_attn_decode_batched_bf16(q, q_batch_stride, q_head_stride, out, out_batch_stride, out_head_stride, n_batch,
                                            group, full, stream_cls, scale, head_dim, workspace, workspace_bytes, stream);
    if (group > 16 || (group & (group - 1))) return DUO_EGROUP;     // the 16 columns hold whole tokens: 1, 2, 4, 8, 16
    if (n_batch == 0) return 0;
    if (((q_token_stride | q_head_stride) & 7) || ((out_token_stride | out_head_stride) & 3)) return DUO_EINVAL;
    if (n_batch > 1 && ((q_batch_stride & 7) || (out_batch_stride & 3))) return DUO_EINVAL;

    MultiParams P;
    P.q = (const bf16_t *)q;
    P.out = (bf16_t *)out;
    P.q_ts = q_token_stride; P.q_hs = q_head_stride; P.q_bs = q_batch_stride;
    P.out_ts = out_token_stride; P.out_hs = out_head_stride; P.out_bs = out_batch_stride;
    P.cls[0] = duo_class_dev(full);
    P.cls[1] = duo_class_dev(stream_cls);
    P.group = group;
    P.n_tokens = n_tokens;
    P.tpb = 16 / group;
    P.scale_log2e = scale * 1.4426950408889634f;
    for (int c = 0; c < 2; ++c) {
        DuoClassDev &C = P.cls[c];
        if (C.n_kv_heads <= 0) { C.n_kv_heads = 0; continue; }
        // segment B is the step's own rows; row blocks of a longer chunk are the prefill entry points' business
        if (C.a.len < 0 || C.b.len != n_tokens || !C.b.k || !C.b.v || (C.a.len > 0 && (!C.a.k || !C.a.v))) return DUO_EINVAL;
        // 16-byte row loads; 32-bit lane offsets inside a 32-key tile
        if (((C.a.token_stride | C.a.head_stride | C.a.batch_stride | C.b.token_stride | C.b.head_stride | C.b.batch_stride) & 7) ||
            C.a.token_stride < 0 || C.a.token_stride > (1ll << 24))
            return DUO_EINVAL;
        if (C.a.len == 0) { C.a = C.b; C.a.len = 0; }      // a valid base; no row is ever read through it
    }
    const int n_q_heads = (P.cls[0].n_kv_heads + P.cls[1].n_kv_heads) * group;
    if (n_q_heads <= 0) return 0;

    const int n_cb = (n_tokens + P.tpb - 1) / P.tpb;        // column blocks: each reads its kv head's rows once
    const int64_t n_rows = (int64_t)n_batch * n_tokens;     // partial areas: one per (batch row, token)
    const int64_t per_split = (int64_t)n_q_heads * (DUO_HEAD_DIM + 2) * (int64_t)sizeof(float) * n_rows;
    const int max_splits = workspace ? (int)std::min<int64_t>(workspace_bytes / per_split, DUO_DECODE_MULTI_MAX_SPLITS) : 0;
    const int ms = DUO_DECODE_MULTI_MAX_SPLITS;
    // the single-token plan, its workgroup budget shared by the batch rows and the column blocks; the workspace does not
    // shape the plan (a workspace-dependent grid would make results depend on the caller's scratch): it holds it or it does not
    const int target = std::max(1, duo_decode_target_wgs() / (n_batch * n_cb));
    const int Ls = P.cls[1].a.len + n_tokens, Lf = P.cls[0].a.len + n_tokens;
    duo_decode_choose_splits(P.cls[1].n_kv_heads, Ls, ms, P.cls[0].n_kv_heads > 0 ? P.cls[1].n_kv_heads : target, P.splits[1]);
    duo_decode_choose_splits(P.cls[0].n_kv_heads, Lf, ms,
                             std::max(target - P.cls[1].n_kv_heads * P.splits[1], P.cls[0].n_kv_heads), P.splits[0]);
    const int need = std::max(P.splits[0], P.splits[1]);
    if (need > 1 && max_splits < need) return DUO_EWORKSPC;
    P.max_splits = need > 1 ? need : 1;
    P.ws_ml = (float *)workspace;
    P.ws_acc = P.ws_ml ? P.ws_ml + (int64_t)n_q_heads * P.max_splits * 2 : nullptr;
    P.ws_row_floats = (int64_t)n_q_heads * P.max_splits * (DUO_HEAD_DIM + 2);
    P.nblk_full = P.cls[0].n_kv_heads * P.splits[0];
    const int nblk = P.nblk_full + P.cls[1].n_kv_heads * P.splits[1];

    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(duo_decode_multi_kernel, dim3(nblk, n_cb, n_batch), dim3(256), 0, st, P);
    DUO_HIP_CHECK_LAUNCH();

    MultiMergeParams M;
    M.ws_ml = P.ws_ml; M.ws_acc = P.ws_acc; M.out = P.out;
    M.out_ts = out_token_stride; M.out_hs = out_head_stride; M.out_bs = out_batch_stride;
    M.max_splits = P.max_splits; M.n_tokens = n_tokens;
    M.ws_row_floats = P.ws_row_floats;
    int n_merge = 0;
    for (int c = 0; c < 2; ++c) {
        M.qh_begin[c] = P.cls[c].q_head_offset;
        M.qh_end[c] = P.cls[c].q_head_offset + P.cls[c].n_kv_heads * group;
        M.splits[c] = P.splits[c];
        if (P.splits[c] > 1) n_merge += P.cls[c].n_kv_heads * group;
    }
    if (n_merge > 0) {
        hipLaunchKernelGGL(duo_decode_multi_merge_kernel, dim3(n_merge, 4, (unsigned)n_rows), dim3(256), 0, st, M);
        DUO_HIP_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int duo_attn_decode_multi_bf16(const void *q, int64_t q_token_stride, int64_t q_head_stride, void *out,
                                          int64_t out_token_stride, int64_t out_head_stride, int32_t n_tokens, int32_t group,
                                          const duo_head_class *full, const duo_head_class *stream_cls, float scale,
                                          int32_t head_dim, void *workspace, int64_t workspace_bytes, void *stream) {
    return duo_attn_decode_multi_batched_bf16(q, 0, q_token_stride, q_head_stride, out, 0, out_token_stride, out_head_stride, 1,
                                              n_tokens, group, full, stream_cls, scale, head_dim, workspace, workspace_bytes,
                                              stream);
}
