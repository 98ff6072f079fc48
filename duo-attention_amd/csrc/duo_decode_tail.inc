// duo_decode_tail.inc — everything behind the scan loop, included textually at the end of duo_decode_scan_kernel
// (duo_decode.hip); kept as a file of its own so the kernel reads as prologue / loop / tail.  Textual on purpose: handing the by-value kernel
// arguments P / CP to a helper by reference makes hipcc copy them to scratch (their dynamically indexed inv_freq tables
// are then no longer read straight from the kernarg segment).
// In scope: P, CP, GT, FUSED, m[], l[], acc[][], qh0, split, splits, ci, kvh, wave, sub, tg, and the batch row's bz,
// out_row, ws_ml_row, ws_acc_row (the single-launch step's ticketed merge is not batched: it runs with one row).
// The wave's four token groups and the workgroup's four waves are combined, the result goes to `out` (single split) or
// to the partial workspace, and — single-launch step / folded streaming update — the merge and the sink+recent pool
// update run here.
    // ---- combine the workgroup's 16 running states — 4 waves x 4 token groups (lanes l, l^16, l^32, l^48 of a wave
    //      hold the same dim slice of different tokens) — through LDS.  (Round 2 folded the four token groups with 80
    //      cross-lane shuffles per wave first: ~2 000 cycles of the epilogue; here every (wave, token group) writes its
    //      state once and the 256 threads fold all 16 with the same rescale arithmetic, two dims each.)
    constexpr int NP = 16;
    __shared__ float s_ml[NP][GT][2];
    __shared__ __attribute__((aligned(16))) float s_acc[NP][GT][DUO_HEAD_DIM];
    {
        const int pi = wave * 4 + tg;
#pragma unroll
        for (int g = 0; g < GT; ++g) {
            if (sub == 0) {
                s_ml[pi][g][0] = m[g];
                s_ml[pi][g][1] = l[g];
            }
            const f32x4 lo = {acc[g][0], acc[g][1], acc[g][2], acc[g][3]};
            const f32x4 hi = {acc[g][4], acc[g][5], acc[g][6], acc[g][7]};
            *reinterpret_cast<f32x4 *>(&s_acc[pi][g][sub * 8]) = lo;
            *reinterpret_cast<f32x4 *>(&s_acc[pi][g][sub * 8 + 4]) = hi;
        }
    }
    DUO_DT(6);
    __syncthreads();
    DUO_DT(7);

    // one thread per (q head, 2 dims) — all 256 threads for a group of 4 q heads; both forms below store the SAME values
    // (the one-launch step is bit-identical to the two-launch step by construction)
    typedef __attribute__((ext_vector_type(2))) float f32x2_tail;
    // (one_launch == 2 — two launches with the streaming-pool update folded in — merges in the NEXT launch: plain stores into
    //  the batch row's own partial area, like the plain two-launch step; the publishing form addresses row 0's area only)
    const bool publish = FUSED && P.one_launch == 1 && splits > 1;
    for (int idx = threadIdx.x; idx < GT * (DUO_HEAD_DIM / 2); idx += 256) {
        const int g = idx >> 6;
        const int d = (idx & 63) * 2;
        float M = s_ml[0][g][0];
#pragma unroll
        for (int i = 1; i < NP; ++i) M = fmaxf(M, s_ml[i][g][0]);
        float Lsum = 0.f;
        f32x2_tail o = {0.f, 0.f};
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const float sc = fast_exp2(s_ml[i][g][0] - M);      // a state that saw no token: exp2(-1e30 - M) = 0
            Lsum = fmaf(s_ml[i][g][1], sc, Lsum);
            const f32x2_tail a = *reinterpret_cast<const f32x2_tail *>(&s_acc[i][g][d]);
            o.x = fmaf(a.x, sc, o.x);
            o.y = fmaf(a.y, sc, o.y);
        }
        const int qh = qh0 + g;
        if (splits == 1) {
            // single split: this workgroup saw every key of the head
            *reinterpret_cast<uint32_t *>(out_row + (int64_t)qh * P.out_head_stride + d) = pack_bf16x2(o.x / Lsum, o.y / Lsum);
        } else if (!publish) {
            const int64_t slot = (int64_t)qh * P.max_splits + split;
            *reinterpret_cast<f32x2_tail *>(ws_acc_row + slot * DUO_HEAD_DIM + d) = o;
            if (d == 0) {
                ws_ml_row[slot * 2 + 0] = M;
                ws_ml_row[slot * 2 + 1] = Lsum;
            }
        } else {
            // Single-launch step: the partial is PUBLISHED to other workgroups of this launch — write-through
            // (sc1) stores, so no release fence (an L2 write-back per workgroup) is needed
            const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)P.ws_ml, 0, P.ws_bytes, 0x00020000);
            const uint32_t acc_base = (uint32_t)((const char *)P.ws_acc - (const char *)P.ws_ml);
            const uint32_t slot = (uint32_t)qh * P.max_splits + split;
            u32x2 ow = {__float_as_uint(o.x), __float_as_uint(o.y)};
            __builtin_amdgcn_raw_buffer_store_b64(ow, rsrc, acc_base + (slot * DUO_HEAD_DIM + d) * 4, 0, 16);
            if (d == 0) {
                const unsigned long long ml = ((unsigned long long)__float_as_uint(Lsum) << 32) | __float_as_uint(M);
                __hip_atomic_store(reinterpret_cast<unsigned long long *>(P.ws_ml + (size_t)slot * 2), ml,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if (publish) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave drains its own stores

    DUO_DT(3);
    DUO_DRT(9);
    // ---- single-launch step: the merge of the partials and the streaming-pool update happen here ---------
    // (grid.y == 1 is guaranteed by the launcher, so the workgroups of a kv head are exactly its `splits`)
    if constexpr (FUSED) {
        if (!P.one_launch) return;
        if (P.one_launch == 2) {
            // two launches, but a streaming head scanned by ONE workgroup updates its pool right here (every read of
            // that head's pool by this launch is this workgroup's own scan, behind the barrier above): the epilogue
            // launch is then the merge alone
            if (splits == 1 && ci == 1 && CP.n_heads > 0) {
                duo_stream_compress_block(CP, 2 * kvh, bz);
                duo_stream_compress_block(CP, 2 * kvh + 1, bz);
            }
            return;
        }
        bool do_compress = false;
        if (splits == 1) {
            // this workgroup saw every cached row of the head; its waves left the scan through the barrier above
            do_compress = ci == 1;
        } else {
            // The partial went out write-through and drained above; after the barrier one lane takes the head's
            // ticket (MI355X inter-workgroup hand-off, form R1).  The LAST min(splits, 4 GT) arrivals of the head
            // stay as mergers: merger j takes the (q head, 32-dim quarter) tasks j, j + NM, ...; every merger
            // first waits until all `splits` partials are published (bounded spin).
            __shared__ int s_ticket;
            int32_t *cnt = P.tickets + 2 * ((ci ? P.cls[0].n_kv_heads : 0) + kvh);
            __syncthreads();
            if (threadIdx.x == 0)
                s_ticket = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            const int n = s_ticket;
            const int n_tasks = 4 * GT;
            const int NM = min(splits, n_tasks);
            if (n < splits - NM) return;
            const int j = n - (splits - NM);
            if (threadIdx.x == 0) {
                int spins = 0;
                while (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < splits) {
                    __builtin_amdgcn_s_sleep(2);
                    if (++spins > kSpinLimit) {   // never seen; better a flagged wrong answer than a hung GPU
                        __hip_atomic_store(P.tickets + kTicketWords - 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        break;
                    }
                }
                // no acquire fence: the partials were stored sc1 and are read back with sc1 loads
            }
            __syncthreads();
            for (int task = j; task < n_tasks; task += NM) {
                duo_decode_merge_task<true>(P.ws_ml, P.ws_acc, P.ws_bytes, P.out, P.out_head_stride, P.max_splits,
                                            qh0 + (task >> 2), task & 3, splits);
                __syncthreads();
            }
            do_compress = ci == 1 && j == 0;   // (a streaming class scanned in splits: an all-streaming layer)
            // the last merger to finish re-arms the head's tickets for the next launch
            if (threadIdx.x == 0) {
                const int d = __hip_atomic_fetch_add(cnt + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (d == NM - 1) {
                    __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(cnt + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        if (do_compress && CP.n_heads > 0) {
            // sink+recent update of this streaming head's K and V rows (every read of the pool by this launch
            // is behind us: this workgroup's own scan, or — split scan — all arrivals of the head)
            duo_stream_compress_block(CP, 2 * kvh, bz);
            duo_stream_compress_block(CP, 2 * kvh + 1, bz);
        }
    }
