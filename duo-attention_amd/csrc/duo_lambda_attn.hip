// Λ-mask ("streaming") attention for retrieval-head training: forward with log-sum-exp, and a deterministic backward.
//
// Query row i sees key j iff j <= i and (j < sink_end or j >= (i / blk - nb + 1) * blk):
//   token mode (reference streaming_attn.py:14-24):  sink_end = sink,        blk = 1,   nb = recent
//   block mode (reference streaming_attn.py:70-108): sink_end = 128 * nsb,   blk = 128, nb = nlb (local blocks, diagonal
//                                                    block included)
// Equivalently key j is seen by rows [j, S) if j < sink_end, else by rows [j, (j / blk + nb) * blk).
//
// Tiles: a workgroup of 4 waves holds 64 PACKED query rows — `rows` = 64 / G consecutive positions x the G q heads of one
// kv head (packed row p = position pos0 + p / G, q head kvh * G + p % G) — so every K/V tile it stages in LDS serves the
// whole group.  Keys come in tiles of 64.  All products run on v_mfma_f32_16x16x32_bf16 (A: lane l holds row l&15,
// k 8(l>>4)..+7; B: k 8(l>>4)..+7, column l&15; C: column l&15, rows 4(l>>4)..+3).  A C-layout tile that must become an A
// operand (P, dS) is staged through a per-wave LDS image.
//
// Forward (lambda_q_kernel<false>): per query tile, the sink tiles [0, ceil(min(sink_end, i1 + 1) / 64)) and then the band
// tiles from max(that, lo(i0) / 64) to i1 / 64 — no key tile is visited twice, so the overlap of sink and band on the first
// rows is counted once.  Masking is element-exact only on tiles that are not wholly visible to every row of the tile.
// fp32 scores and online softmax, P rounded to bf16 before P.V, l summed from the fp32 P, LSE = m * scale + ln l.
//
// Backward (FA2 convention, P recomputed from Q, K and the LSE):
//   (a) lambda_delta_kernel:  delta = rowsum(dO o O) in fp32;
//   (b) lambda_q_kernel<true>: dQ = scale * sum_j dS K over the forward's key set (query-major, no sum across workgroups);
//   (c) lambda_kv_kernel: dK = scale * sum_i dS^T Q, dV = sum_i P^T dO, key-major.  A band key tile is seen by at most
//       recent + 64 rows; a sink key tile by every later row, so its query range is cut into pieces of QSPLIT positions,
//       each piece leaves fp32 partials, and lambda_kv_reduce_kernel sums them in piece order.  No float atomics anywhere:
//       a rerun (or a recompute under activation checkpointing) is bit-identical.
// dS = P o (dP - delta) in fp32, rounded to bf16 before the dQ and dK products; P rounded to bf16 before the dV product.
// All stores are vector-memory stores issued by plain C++.
#include <algorithm>
#include "duo_common.h"

namespace {

constexpr int LQ = 64;        // packed query rows per workgroup (4 waves x 16)
constexpr int LK = 64;        // keys per tile
constexpr int LDR = 136;      // row stride (elements) of a row-major [64][128] LDS tile (+16 B: spreads the banks)
constexpr int LDT = 72;       // row stride of a transposed [128][64] LDS tile and of the per-wave [16][64] staging
constexpr int QSPLIT = 512;   // query positions per piece of a sink key tile's dK/dV pass

typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;

struct LamParams {
    const bf16_t *q, *k, *v, *dout, *o;
    int64_t q_bs, q_ts, q_hs, k_bs, k_ts, k_hs, v_bs, v_ts, v_hs, d_bs, d_ts, d_hs;
    bf16_t *out;          // forward: attention output; backward: dQ        ([B, S, Hq, D] contiguous)
    bf16_t *dk, *dv;      // [B, S, Hkv, D] contiguous
    float *lse;           // [B, Hq, S]
    float *delta;         // [B, Hq, S]
    float *part;          // [B][Hkv][n_sink_tiles][nsplit][2][64][128] fp32 partials of the sink key tiles
    int32_t S, Hq, Hkv, G, rows;
    int32_t sink_end, blk, nb;
    int32_t n_sink_tiles, nsplit;
    float scale, scale_log2e;
};

__device__ __forceinline__ int band_lo(const LamParams &P, int i) { return (i / P.blk - P.nb + 1) * P.blk; }
__device__ __forceinline__ int band_hi(const LamParams &P, int j) { return (j / P.blk + P.nb) * P.blk; }
// i < 0 marks a padding row: it sees nothing
__device__ __forceinline__ bool lam_visible(const LamParams &P, int i, int j) {
    return j <= i && (j < P.sink_end || j >= band_lo(P, i));
}

__device__ __forceinline__ f32x4 mfma16(const bf16x8 &a, const bf16x8 &b, const f32x4 &c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float row16_allreduce_max(float x) {
    x = fmaxf(x, dpp_mov<DUO_DPP_QUAD_XOR1>(x));
    x = fmaxf(x, dpp_mov<DUO_DPP_QUAD_XOR2>(x));
    x = fmaxf(x, dpp_mov<DUO_DPP_ROW_HALF_MIRROR>(x));
    x = fmaxf(x, dpp_mov<DUO_DPP_ROW_MIRROR>(x));
    return x;
}

__device__ __forceinline__ u32x4 load16(const bf16_t *p) { return *reinterpret_cast<const u32x4 *>(p); }
__device__ __forceinline__ bf16x8 as_frag(const u32x4 &w) { return *reinterpret_cast<const bf16x8 *>(&w); }

// one 16-byte chunk (8 elements of a row) into a row-major and/or a transposed LDS image
__device__ __forceinline__ void put_chunk(bf16_t *rm, bf16_t *tr, int row, int ch, const u32x4 &val) {
    if (rm) *reinterpret_cast<u32x4 *>(rm + row * LDR + ch * 8) = val;
    if (tr) {
        const u16x8 e = *reinterpret_cast<const u16x8 *>(&val);
#pragma unroll
        for (int x = 0; x < 8; ++x) tr[(ch * 8 + x) * LDT + row] = e[x];
    }
}

// lane's B fragment X[row0 + (l & 15)][32 ks + 8 (l >> 4) ..] of a row-major image (B of a product summing over d)
__device__ __forceinline__ bf16x8 rm_frag(const bf16_t *rm, int row0, int ks, int lr, int lh) {
    return as_frag(*reinterpret_cast<const u32x4 *>(rm + (row0 + lr) * LDR + 32 * ks + 8 * lh));
}
// lane's B fragment X[k = 32 ks + 8 (l >> 4) ..][col = 16 db + (l & 15)] of a transposed image (B of a product summing
// over the 64 rows of the tile)
__device__ __forceinline__ bf16x8 tr_frag(const bf16_t *tr, int db, int ks, int lr, int lh) {
    return as_frag(*reinterpret_cast<const u32x4 *>(tr + (16 * db + lr) * LDT + 32 * ks + 8 * lh));
}
// C layout [16][64] (4 column blocks) -> bf16 staging image of this wave; then the A fragment of k-step ks
__device__ __forceinline__ void stage_c(bf16_t *st, const f32x4 (&c)[4], int lr, int lh) {
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) st[(4 * lh + r) * LDT + 16 * cb + lr] = (bf16_t)f32_to_bf16_bits(c[cb][r]);
}
__device__ __forceinline__ bf16x8 st_frag(const bf16_t *st, int ks, int lr, int lh) {
    return as_frag(*reinterpret_cast<const u32x4 *>(st + lr * LDT + 32 * ks + 8 * lh));
}

// stage key rows [k0, k0 + 64) of one kv head (rows >= S are zero): row-major image `rm` and/or transposed image `tr`
__device__ __forceinline__ void stage_keys(const bf16_t *src, int64_t ts, int k0, int S, bf16_t *rm, bf16_t *tr, int tid) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int c = tid + 256 * u, row = c >> 4, ch = c & 15;
        u32x4 val = {0u, 0u, 0u, 0u};
        if (k0 + row < S) val = load16(src + (int64_t)(k0 + row) * ts + ch * 8);
        put_chunk(rm, tr, row, ch, val);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// query-major pass: forward (BWD = false) or dQ (BWD = true).  grid (query tiles, Hkv, B), 256 threads.
template <bool BWD>
__global__ __launch_bounds__(256) void lambda_q_kernel(LamParams P) {
    __shared__ __attribute__((aligned(16))) bf16_t k_rm[LK * LDR];            // K rows (S = Q K^T)
    __shared__ __attribute__((aligned(16))) bf16_t x_tr[DUO_HEAD_DIM * LDT];  // forward: V^T; backward: K^T
    __shared__ __attribute__((aligned(16))) bf16_t v_rm[BWD ? LK * LDR : 8];  // backward: V rows (dP = dO V^T)
    __shared__ __attribute__((aligned(16))) bf16_t stg[4 * 16 * LDT];         // per-wave P / dS staging

    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lr = l & 15, lh = l >> 4;
    const int kvh = blockIdx.y, b = blockIdx.z, G = P.G, S = P.S;
    const int pos0 = blockIdx.x * P.rows;
    const int i0 = pos0, i1 = min(pos0 + P.rows, S) - 1;
    bf16_t *st = stg + w * 16 * LDT;

    // A-operand row of this lane (Q, dO)
    const int pa = 16 * w + lr;
    const int posA = pos0 + pa / G, qhA = kvh * G + pa % G;
    const bool validA = pa < P.rows * G && posA < S;
    bf16x8 qf[4], df[4];
    const bf16_t *qrow = P.q + (int64_t)b * P.q_bs + (int64_t)posA * P.q_ts + (int64_t)qhA * P.q_hs;
    const bf16_t *drow = BWD ? P.dout + (int64_t)b * P.d_bs + (int64_t)posA * P.d_ts + (int64_t)qhA * P.d_hs : nullptr;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        u32x4 z = {0u, 0u, 0u, 0u};
        qf[ks] = as_frag(validA ? load16(qrow + 32 * ks + 8 * lh) : z);
        if constexpr (BWD) df[ks] = as_frag(validA ? load16(drow + 32 * ks + 8 * lh) : z);
    }
    // C-layout rows of this lane
    int posC[4], qhC[4];
    float lseC[4], delC[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int pc = 16 * w + 4 * lh + r;
        const int pos = pos0 + pc / G;
        posC[r] = (pc < P.rows * G && pos < S) ? pos : -1;
        qhC[r] = kvh * G + pc % G;
        lseC[r] = 0.f;
        delC[r] = 0.f;
        if constexpr (BWD) {
            if (posC[r] >= 0) {
                const int64_t li = ((int64_t)b * P.Hq + qhC[r]) * S + posC[r];
                lseC[r] = P.lse[li] * 1.4426950408889634f;
                delC[r] = P.delta[li];
            }
        }
    }

    f32x4 acc[8];
#pragma unroll
    for (int db = 0; db < 8; ++db) acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m[4], lsum[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        m[r] = -INFINITY;
        lsum[r] = 0.f;
    }

    const bf16_t *kbase = P.k + (int64_t)b * P.k_bs + (int64_t)kvh * P.k_hs;
    const bf16_t *vbase = P.v + (int64_t)b * P.v_bs + (int64_t)kvh * P.v_hs;
    const int n_sink = (min(P.sink_end, i1 + 1) + LK - 1) / LK;
    const int bt0 = max(n_sink, max(band_lo(P, i0), 0) / LK), bt1 = i1 / LK;
    const int n_tiles = n_sink + max(0, bt1 - bt0 + 1);
    const float c = P.scale_log2e;

    for (int it = 0; it < n_tiles; ++it) {
        const int t = it < n_sink ? it : bt0 + (it - n_sink);
        const int k0 = t * LK;
        __syncthreads();
        if constexpr (BWD) {
            stage_keys(kbase, P.k_ts, k0, S, k_rm, x_tr, tid);
            stage_keys(vbase, P.v_ts, k0, S, v_rm, nullptr, tid);
        } else {
            stage_keys(kbase, P.k_ts, k0, S, k_rm, nullptr, tid);
            stage_keys(vbase, P.v_ts, k0, S, nullptr, x_tr, tid);
        }
        __syncthreads();
        const bool full = (k0 + LK - 1 <= i0) && (k0 + LK <= P.sink_end || k0 >= band_lo(P, i1));

        f32x4 s[4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            s[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) s[cb] = mfma16(qf[ks], rm_frag(k_rm, 16 * cb, ks, lr, lh), s[cb]);
        }
        if (!full) {
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (!lam_visible(P, posC[r], k0 + 16 * cb + lr)) s[cb][r] = -INFINITY;
        }

        if constexpr (!BWD) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float mx = fmaxf(fmaxf(s[0][r], s[1][r]), fmaxf(s[2][r], s[3][r]));
                mx = row16_allreduce_max(mx);
                const float mn = fmaxf(m[r], mx);
                const float mu = mn == -INFINITY ? 0.f : mn;     // a row with nothing seen yet: every term is 0
                const float alpha = fast_exp2((m[r] - mu) * c);
                m[r] = mn;
                float ps = 0.f;
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    s[cb][r] = fast_exp2((s[cb][r] - mu) * c);
                    ps += s[cb][r];
                }
                lsum[r] = lsum[r] * alpha + ps;
#pragma unroll
                for (int db = 0; db < 8; ++db) acc[db][r] *= alpha;
            }
            stage_c(st, s, lr, lh);
            __syncthreads();
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bf16x8 pa8 = st_frag(st, ks, lr, lh);
#pragma unroll
                for (int db = 0; db < 8; ++db) acc[db] = mfma16(pa8, tr_frag(x_tr, db, ks, lr, lh), acc[db]);
            }
        } else {
            f32x4 dp[4];
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                dp[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) dp[cb] = mfma16(df[ks], rm_frag(v_rm, 16 * cb, ks, lr, lh), dp[cb]);
            }
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = fast_exp2(s[cb][r] * c - lseC[r]);
                    s[cb][r] = p * (dp[cb][r] - delC[r]);
                }
            stage_c(st, s, lr, lh);
            __syncthreads();
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bf16x8 da8 = st_frag(st, ks, lr, lh);
#pragma unroll
                for (int db = 0; db < 8; ++db) acc[db] = mfma16(da8, tr_frag(x_tr, db, ks, lr, lh), acc[db]);
            }
        }
    }

#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float mul;
        if constexpr (!BWD) {
            const float L = row16_allreduce_sum(lsum[r]);
            mul = L > 0.f ? 1.f / L : 0.f;
            if (posC[r] >= 0 && lr == 0)
                P.lse[((int64_t)b * P.Hq + qhC[r]) * S + posC[r]] = m[r] * P.scale + __logf(L);
        } else {
            mul = P.scale;
        }
        if (posC[r] < 0) continue;
        bf16_t *orow = P.out + (((int64_t)b * S + posC[r]) * P.Hq + qhC[r]) * DUO_HEAD_DIM;
#pragma unroll
        for (int db = 0; db < 8; ++db) orow[16 * db + lr] = (bf16_t)f32_to_bf16_bits(acc[db][r] * mul);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// delta = rowsum(dO o O): one wave per (batch, position, q head) row; grid ceil(rows / 4), 256 threads
__global__ __launch_bounds__(256) void lambda_delta_kernel(LamParams P, int64_t n_rows) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int l = threadIdx.x & 63;
    if (row >= n_rows) return;
    const int h = (int)(row % P.Hq);
    const int64_t bt = row / P.Hq;
    const int pos = (int)(bt % P.S), b = (int)(bt / P.S);
    const uint32_t ow = *reinterpret_cast<const uint32_t *>(P.o + row * DUO_HEAD_DIM + 2 * l);
    const uint32_t dw = *reinterpret_cast<const uint32_t *>(P.dout + (int64_t)b * P.d_bs + (int64_t)pos * P.d_ts +
                                                             (int64_t)h * P.d_hs + 2 * l);
    float x = bf16_lo(ow) * bf16_lo(dw) + bf16_hi(ow) * bf16_hi(dw);
    x = row16_allreduce_sum(x);
    x += __shfl_xor(x, 16);
    x += __shfl_xor(x, 32);
    if (l == 0) P.delta[((int64_t)b * P.Hq + h) * P.S + pos] = x;
}

// ---------------------------------------------------------------------------------------------------------------------
// key-major dK / dV pass.  grid (n_sink_tiles * nsplit + band tiles, Hkv, B), 256 threads; wave w owns keys
// k0 + 16 w .. + 15 of the tile and sweeps the packed query rows of its range.
__global__ __launch_bounds__(256) void lambda_kv_kernel(LamParams P) {
    __shared__ __attribute__((aligned(16))) bf16_t q_rm[LQ * LDR];
    __shared__ __attribute__((aligned(16))) bf16_t q_tr[DUO_HEAD_DIM * LDT];
    __shared__ __attribute__((aligned(16))) bf16_t d_rm[LQ * LDR];
    __shared__ __attribute__((aligned(16))) bf16_t d_tr[DUO_HEAD_DIM * LDT];
    __shared__ __attribute__((aligned(16))) bf16_t stg_p[4 * 16 * LDT];
    __shared__ __attribute__((aligned(16))) bf16_t stg_s[4 * 16 * LDT];
    __shared__ float lse_s[LQ], del_s[LQ];
    __shared__ int pos_s[LQ];

    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lr = l & 15, lh = l >> 4;
    const int kvh = blockIdx.y, b = blockIdx.z, G = P.G, S = P.S;
    const int n_sp = P.n_sink_tiles * P.nsplit;
    const int item = blockIdx.x;
    const bool sink_piece = item < n_sp;
    const int t = sink_piece ? item / P.nsplit : P.n_sink_tiles + (item - n_sp);
    const int piece = sink_piece ? item % P.nsplit : 0;
    const int k0 = t * LK;
    int qa, qb;
    if (sink_piece) {
        qa = max(k0, piece * QSPLIT);
        qb = min(S, (piece + 1) * QSPLIT);
    } else {
        qa = k0;
        qb = min(S, band_hi(P, min(k0 + LK, S) - 1));
    }

    // K and V rows of this wave as A fragments
    const int keyA = k0 + 16 * w + lr;
    bf16x8 kf[4], vf[4];
    {
        const bf16_t *kr = P.k + (int64_t)b * P.k_bs + (int64_t)keyA * P.k_ts + (int64_t)kvh * P.k_hs;
        const bf16_t *vr = P.v + (int64_t)b * P.v_bs + (int64_t)keyA * P.v_ts + (int64_t)kvh * P.v_hs;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            u32x4 z = {0u, 0u, 0u, 0u};
            kf[ks] = as_frag(keyA < S ? load16(kr + 32 * ks + 8 * lh) : z);
            vf[ks] = as_frag(keyA < S ? load16(vr + 32 * ks + 8 * lh) : z);
        }
    }
    int keyC[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) keyC[r] = k0 + 16 * w + 4 * lh + r;

    f32x4 dka[8], dva[8];
#pragma unroll
    for (int db = 0; db < 8; ++db) {
        dka[db] = f32x4{0.f, 0.f, 0.f, 0.f};
        dva[db] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const float c = P.scale_log2e;
    bf16_t *sp = stg_p + w * 16 * LDT, *ss = stg_s + w * 16 * LDT;

    for (int t0 = qa; t0 < qb; t0 += P.rows) {
        const int tlast = min(t0 + P.rows, qb) - 1;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int cidx = tid + 256 * u, row = cidx >> 4, ch = cidx & 15;
            const int pos = t0 + row / G, qh = kvh * G + row % G;
            const bool ok = row < P.rows * G && pos <= tlast;
            u32x4 qv = {0u, 0u, 0u, 0u}, dv = {0u, 0u, 0u, 0u};
            if (ok) {
                qv = load16(P.q + (int64_t)b * P.q_bs + (int64_t)pos * P.q_ts + (int64_t)qh * P.q_hs + ch * 8);
                dv = load16(P.dout + (int64_t)b * P.d_bs + (int64_t)pos * P.d_ts + (int64_t)qh * P.d_hs + ch * 8);
            }
            put_chunk(q_rm, q_tr, row, ch, qv);
            put_chunk(d_rm, d_tr, row, ch, dv);
        }
        if (tid < LQ) {
            const int pos = t0 + tid / G, qh = kvh * G + tid % G;
            const bool ok = tid < P.rows * G && pos <= tlast;
            const int64_t li = ((int64_t)b * P.Hq + qh) * S + pos;
            pos_s[tid] = ok ? pos : -1;
            lse_s[tid] = ok ? P.lse[li] * 1.4426950408889634f : 0.f;
            del_s[tid] = ok ? P.delta[li] : 0.f;
        }
        __syncthreads();
        const bool full = P.rows * G == LQ && t0 + P.rows - 1 <= tlast && (k0 + LK - 1 <= t0) &&
                          (k0 + LK <= P.sink_end || k0 >= band_lo(P, tlast));

        f32x4 pt[4], dpt[4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            pt[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
            dpt[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                pt[cb] = mfma16(kf[ks], rm_frag(q_rm, 16 * cb, ks, lr, lh), pt[cb]);
                dpt[cb] = mfma16(vf[ks], rm_frag(d_rm, 16 * cb, ks, lr, lh), dpt[cb]);
            }
        }
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            const int qr = 16 * cb + lr;
            const float ls = lse_s[qr], de = del_s[qr];
            const int pos = pos_s[qr];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float p = fast_exp2(pt[cb][r] * c - ls);
                if (!full && !lam_visible(P, pos, keyC[r])) p = 0.f;
                pt[cb][r] = p;
                dpt[cb][r] = p * (dpt[cb][r] - de);
            }
        }
        stage_c(sp, pt, lr, lh);
        stage_c(ss, dpt, lr, lh);
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 pa8 = st_frag(sp, ks, lr, lh);
            const bf16x8 sa8 = st_frag(ss, ks, lr, lh);
#pragma unroll
            for (int db = 0; db < 8; ++db) {
                dva[db] = mfma16(pa8, tr_frag(d_tr, db, ks, lr, lh), dva[db]);
                dka[db] = mfma16(sa8, tr_frag(q_tr, db, ks, lr, lh), dka[db]);
            }
        }
    }

    if (sink_piece) {
        float *base = P.part + ((((int64_t)b * P.Hkv + kvh) * P.n_sink_tiles + t) * P.nsplit + piece) * 2 * LK * DUO_HEAD_DIM;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int kl = 16 * w + 4 * lh + r;
#pragma unroll
            for (int db = 0; db < 8; ++db) {
                base[kl * DUO_HEAD_DIM + 16 * db + lr] = dka[db][r] * P.scale;
                base[(LK + kl) * DUO_HEAD_DIM + 16 * db + lr] = dva[db][r];
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (keyC[r] >= S) continue;
            const int64_t o = (((int64_t)b * S + keyC[r]) * P.Hkv + kvh) * DUO_HEAD_DIM;
#pragma unroll
            for (int db = 0; db < 8; ++db) {
                P.dk[o + 16 * db + lr] = (bf16_t)f32_to_bf16_bits(dka[db][r] * P.scale);
                P.dv[o + 16 * db + lr] = (bf16_t)f32_to_bf16_bits(dva[db][r]);
            }
        }
    }
}

// sink key tiles: sum the nsplit partials in piece order.  grid (n_sink_tiles * 8, Hkv, B): 8 key rows per workgroup
__global__ __launch_bounds__(256) void lambda_kv_reduce_kernel(LamParams P) {
    const int kvh = blockIdx.y, b = blockIdx.z;
    const int t = blockIdx.x >> 3, r0 = (blockIdx.x & 7) * 8;
    const float *base = P.part + (((int64_t)b * P.Hkv + kvh) * P.n_sink_tiles + t) * P.nsplit * 2 * LK * DUO_HEAD_DIM;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int o = threadIdx.x + 256 * u;          // [which][8 rows][128]
        const int which = o >> 10, row = r0 + ((o >> 7) & 7), d = o & 127;
        const int key = t * LK + row;
        if (key >= P.S) continue;
        const float *src = base + (which * LK + row) * DUO_HEAD_DIM + d;
        float acc = 0.f;
        for (int s = 0; s < P.nsplit; ++s) acc += src[(int64_t)s * 2 * LK * DUO_HEAD_DIM];
        bf16_t *dst = (which ? P.dv : P.dk) + (((int64_t)b * P.S + key) * P.Hkv + kvh) * DUO_HEAD_DIM + d;
        *dst = (bf16_t)f32_to_bf16_bits(acc);
    }
}

bool lam_aligned(const void *p) { return ((uintptr_t)p & 15) == 0; }
bool lam_stride_ok(int64_t s) { return s >= 0 && (s & 7) == 0; }

int lam_setup(LamParams &P, int32_t B, int32_t S, int32_t Hq, int32_t Hkv, int32_t head_dim, int32_t sink, int32_t recent,
              int32_t block_mode, float scale) {
    P = LamParams{};
    if (head_dim != DUO_HEAD_DIM) return DUO_EHEADDIM;
    if (B <= 0 || S <= 0 || Hq <= 0 || Hkv <= 0 || sink < 0 || recent < 0 || (block_mode != 0 && block_mode != 1))
        return DUO_EINVAL;
    if (Hq % Hkv || Hq / Hkv > LQ) return DUO_EGROUP;
    if (sink == 0 && recent == 0) return DUO_EINVAL;       // a row would see no key
    P.S = S;
    P.Hq = Hq;
    P.Hkv = Hkv;
    P.G = Hq / Hkv;
    P.rows = LQ / P.G;
    P.blk = block_mode ? 128 : 1;
    // clamped so that no index overflows; the visible sets are unchanged (no key lies at or past S)
    P.sink_end = (int32_t)std::min<int64_t>((int64_t)sink * P.blk, S);
    P.nb = (int32_t)std::min<int64_t>(recent, S / P.blk + 2);
    P.n_sink_tiles = (P.sink_end + LK - 1) / LK;
    P.nsplit = (S + QSPLIT - 1) / QSPLIT;
    P.scale = scale;
    P.scale_log2e = scale * 1.4426950408889634f;
    return 0;
}

}  // namespace

extern "C" int64_t duo_lambda_attn_bwd_workspace_bytes(int32_t B, int32_t S, int32_t Hq, int32_t Hkv, int32_t sink,
                                                       int32_t recent, int32_t block_mode) {
    LamParams P;
    const int e = lam_setup(P, B, S, Hq, Hkv, DUO_HEAD_DIM, sink, recent, block_mode, 1.f);
    if (e) return e;
    const int64_t delta = (int64_t)B * Hq * S;
    const int64_t part = (int64_t)B * Hkv * P.n_sink_tiles * P.nsplit * 2 * LK * DUO_HEAD_DIM;
    return (delta + 3) / 4 * 16 + part * 4;
}

extern "C" int duo_lambda_attn_fwd_bf16(const void *q, int64_t q_batch_stride, int64_t q_token_stride, int64_t q_head_stride,
                                        const void *k, int64_t k_batch_stride, int64_t k_token_stride, int64_t k_head_stride,
                                        const void *v, int64_t v_batch_stride, int64_t v_token_stride, int64_t v_head_stride,
                                        void *out, float *lse, int32_t B, int32_t S, int32_t Hq, int32_t Hkv,
                                        int32_t head_dim, int32_t sink, int32_t recent, int32_t block_mode, float scale,
                                        void *stream) {
    LamParams P;
    const int e = lam_setup(P, B, S, Hq, Hkv, head_dim, sink, recent, block_mode, scale);
    if (e) return e;
    if (!q || !k || !v || !out || !lse || !lam_aligned(q) || !lam_aligned(k) || !lam_aligned(v) || !lam_aligned(out))
        return DUO_EINVAL;
    for (int64_t s : {q_batch_stride, q_token_stride, q_head_stride, k_batch_stride, k_token_stride, k_head_stride,
                      v_batch_stride, v_token_stride, v_head_stride})
        if (!lam_stride_ok(s)) return DUO_EINVAL;
    P.q = (const bf16_t *)q;
    P.k = (const bf16_t *)k;
    P.v = (const bf16_t *)v;
    P.q_bs = q_batch_stride; P.q_ts = q_token_stride; P.q_hs = q_head_stride;
    P.k_bs = k_batch_stride; P.k_ts = k_token_stride; P.k_hs = k_head_stride;
    P.v_bs = v_batch_stride; P.v_ts = v_token_stride; P.v_hs = v_head_stride;
    P.out = (bf16_t *)out;
    P.lse = lse;
    hipLaunchKernelGGL(lambda_q_kernel<false>, dim3((S + P.rows - 1) / P.rows, Hkv, B), dim3(256), 0, (hipStream_t)stream, P);
    DUO_HIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int duo_lambda_attn_bwd_bf16(const void *q, int64_t q_batch_stride, int64_t q_token_stride, int64_t q_head_stride,
                                        const void *k, int64_t k_batch_stride, int64_t k_token_stride, int64_t k_head_stride,
                                        const void *v, int64_t v_batch_stride, int64_t v_token_stride, int64_t v_head_stride,
                                        const void *out, const void *dout, int64_t do_batch_stride, int64_t do_token_stride,
                                        int64_t do_head_stride, const float *lse, void *dq, void *dk, void *dv,
                                        void *workspace, int64_t workspace_bytes, int32_t B, int32_t S, int32_t Hq,
                                        int32_t Hkv, int32_t head_dim, int32_t sink, int32_t recent, int32_t block_mode,
                                        float scale, void *stream) {
    LamParams P;
    const int e = lam_setup(P, B, S, Hq, Hkv, head_dim, sink, recent, block_mode, scale);
    if (e) return e;
    if (!q || !k || !v || !out || !dout || !lse || !dq || !dk || !dv || !workspace) return DUO_EINVAL;
    for (const void *p : {q, k, v, out, dout, (const void *)dq, (const void *)dk, (const void *)dv, (const void *)workspace})
        if (!lam_aligned(p)) return DUO_EINVAL;
    for (int64_t s : {q_batch_stride, q_token_stride, q_head_stride, k_batch_stride, k_token_stride, k_head_stride,
                      v_batch_stride, v_token_stride, v_head_stride, do_batch_stride, do_token_stride, do_head_stride})
        if (!lam_stride_ok(s)) return DUO_EINVAL;
    if (workspace_bytes < duo_lambda_attn_bwd_workspace_bytes(B, S, Hq, Hkv, sink, recent, block_mode)) return DUO_EWORKSPC;
    P.q = (const bf16_t *)q;
    P.k = (const bf16_t *)k;
    P.v = (const bf16_t *)v;
    P.o = (const bf16_t *)out;
    P.dout = (const bf16_t *)dout;
    P.q_bs = q_batch_stride; P.q_ts = q_token_stride; P.q_hs = q_head_stride;
    P.k_bs = k_batch_stride; P.k_ts = k_token_stride; P.k_hs = k_head_stride;
    P.v_bs = v_batch_stride; P.v_ts = v_token_stride; P.v_hs = v_head_stride;
    P.d_bs = do_batch_stride; P.d_ts = do_token_stride; P.d_hs = do_head_stride;
    P.lse = const_cast<float *>(lse);
    P.delta = (float *)workspace;
    P.part = (float *)((char *)workspace + ((int64_t)B * Hq * S + 3) / 4 * 16);
    P.out = (bf16_t *)dq;
    P.dk = (bf16_t *)dk;
    P.dv = (bf16_t *)dv;
    hipStream_t st = (hipStream_t)stream;
    const int64_t n_rows = (int64_t)B * S * Hq;
    hipLaunchKernelGGL(lambda_delta_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, st, P, n_rows);
    DUO_HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL(lambda_q_kernel<true>, dim3((S + P.rows - 1) / P.rows, Hkv, B), dim3(256), 0, st, P);
    DUO_HIP_CHECK_LAUNCH();
    const int n_key_tiles = (S + LK - 1) / LK;
    const int n_items = P.n_sink_tiles * P.nsplit + (n_key_tiles - P.n_sink_tiles);
    hipLaunchKernelGGL(lambda_kv_kernel, dim3(n_items, Hkv, B), dim3(256), 0, st, P);
    DUO_HIP_CHECK_LAUNCH();
    if (P.n_sink_tiles > 0) {
        hipLaunchKernelGGL(lambda_kv_reduce_kernel, dim3(P.n_sink_tiles * 8, Hkv, B), dim3(256), 0, st, P);
        DUO_HIP_CHECK_LAUNCH();
    }
    return 0;
}
