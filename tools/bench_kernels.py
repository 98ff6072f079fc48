#!/usr/bin/env python3
"""Micro-benchmark of the two attention kernels alone (for A/B work and PMC passes).

    python tools/bench_kernels.py prefill --nf 4 --past 65536 --chunk 16384 --reps 5
    python tools/bench_kernels.py decode  --ctx 131072 --reps 20        # all 32 layers of the bench pattern
    python tools/bench_kernels.py decode_int4 --ctx 1048576 --q-len 2 4 16   # one layer: a T-token step on the packed pools
                                                                        # against get() + fp16 prefill and the 1-token decode
    python tools/bench_kernels.py decode --ctx 131072 --nf 4 --q-len 1 2 4 8 16 32 64     # one layer: a T-token step on the bf16 pools,
                                                                        # split-KV stream vs the prefill kernel vs the 1-token decode
Prints one JSON line per case: avg ms, algorithmic TFLOP/s or GB/s.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "duo-attention_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

HQ, HKV, D, W = 32, 8, 128, 384


def pools(n_heads, rows, dev, g):
    k = torch.randn(n_heads, rows, D, generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16).permute(1, 0, 2)
    v = torch.randn(n_heads, rows, D, generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16).permute(1, 0, 2)
    return k, v


def time_it(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    evs = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    ts = sorted(x.elapsed_time(y) for x, y in evs)
    return sum(ts) / len(ts), ts[0], ts[len(ts) // 2]


def int4_multi_token(a, dev, g):
    """One layer of the INT4 dual cache (--nf retrieval + 8 - nf streaming kv heads, group 4, sink 128 + recent 256) holding
    --ctx rows, the step's T rows included.  Per T, alternating in this process after a warm-up of each:
      single  decode_attention            the existing one-token launch (the yardstick for a one-pass step)
      multi   multi_token_attention       the T-token step on the packed pools
      parent  prefill_attention           get() (both pools dequantised to fp16 scratch) + the fp16 prefill launch
    Prints one JSON line per T: median / min / max ms of each, the ratios of the medians, the fp16 scratch of `parent`."""
    import types

    from duo_attn.int4_kv import DuoAttentionStaticINT4KVCache

    class Shape(torch.nn.Module):      # what the cache reads of a model: device / dtype of a parameter, the head counts
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1, device=dev, dtype=torch.float16))
            self.config = types.SimpleNamespace(num_hidden_layers=1, num_attention_heads=HQ, num_key_value_heads=HKV,
                                                head_dim=D, hidden_size=HQ * D)

    N, sink, recent, t_max = a.ctx, 128, 256, max(a.q_len)
    heads = [[1.0] * a.nf + [0.0] * (HKV - a.nf)]
    kv = DuoAttentionStaticINT4KVCache(Shape(), heads, 1, N, sink, recent, t_max, multi_token_decode=True)
    for c in (kv.full_key_caches[0], kv.full_value_caches[0], kv.streaming_key_caches[0], kv.streaming_value_caches[0]):
        if c.quantized_data.numel():
            c.quantized_data.random_(0, 256, generator=g)
            c.scale_zero.copy_((torch.rand(c.scale_zero.shape, generator=g, device=dev) * 0.3 + 0.01).to(torch.float16))
    kv.kv_seq_len_list[0] = N

    def timed(fn):
        x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        x.record()
        fn()
        y.record()
        return x, y

    for T in a.q_len:
        kv.streaming_kv_seq_len_list[0] = sink + recent + T       # the window was full, then the step's rows were put
        q = torch.randn(1, T, HQ, D, generator=g, device=dev).to(torch.float16)
        kn = torch.randn(1, T, HKV, D, generator=g, device=dev).to(torch.float16)
        routes = {"single": lambda: kv.decode_attention(0, q[:, :1]),
                  "multi": lambda: kv.multi_token_attention(0, q),
                  "parent": lambda: kv.prefill_attention(0, q, kn, kn)}
        for fn in routes.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        evs = {name: [] for name in routes}
        for _ in range(max(a.reps, 5)):
            for name, fn in routes.items():
                evs[name].append(timed(fn))
        torch.cuda.synchronize()
        ms = {name: sorted(x.elapsed_time(y) for x, y in e) for name, e in evs.items()}
        med = {name: t[len(t) // 2] for name, t in ms.items()}
        print(json.dumps({"case": f"int4 step ctx={N} nf={a.nf} T={T}",
                          **{f"{name}_ms": {"median": round(med[name], 4), "min": round(t[0], 4), "max": round(t[-1], 4)}
                             for name, t in ms.items()},
                          "multi_over_single": round(med["multi"] / med["single"], 3),
                          "parent_over_multi": round(med["parent"] / med["multi"], 3),
                          "parent_scratch_MB": round(sum(b.numel() for b in kv._scratch.values()) * 2 / 1e6, 1)}), flush=True)


def bf16_multi_token(a, be, dev, g):
    """One layer of the bf16 dual cache (--nf retrieval + 8 - nf streaming kv heads, group 4, a full 384-row streaming window)
    whose retrieval pool holds --ctx rows, the step's T rows included.  Per T, alternating in this process after a warm-up of
    each:
      single  attention (T = 1)    the existing one-token split-KV scan (the yardstick for a one-pass step)
      multi   attention_multi      the T-token step on the split-KV matrix-core stream (duo_decode_multi_kernel)
      parent  attention            the same step on the prefill kernel — the route every q_len > 1 took before
    Prints one JSON line per T: median / min / max ms of each and the ratios of the medians."""
    N, G, scale = a.ctx, HQ // HKV, D ** -0.5
    nf, ns = a.nf, HKV - a.nf
    fk, fv = pools(max(nf, 1), N, dev, g)
    sk, sv = pools(max(ns, 1), W, dev, g)

    def timed(fn):
        x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        x.record()
        fn()
        y.record()
        return x, y

    def classes(T, kn, vn):
        full = (nf, 0, (fk[:N - T, :nf], fv[:N - T, :nf]), (fk[N - T:N, :nf], fv[N - T:N, :nf])) if nf else None
        stream = (ns, nf * G, (sk[:, :ns], sv[:, :ns]), (kn[:T, nf:], vn[:T, nf:])) if ns else None
        return full, stream

    for T in a.q_len:
        q = torch.randn(T, HQ, D, generator=g, device=dev).to(torch.bfloat16)
        kn, vn = pools(HKV, T, dev, g)
        out = torch.empty_like(q)
        one, many = classes(1, kn, vn), classes(T, kn, vn)
        routes = {"single": lambda: be.attention(q[:1], out[:1], G, *one, scale),
                  "multi": lambda: be.attention_multi(q, out, G, *many, scale),
                  "parent": lambda: be.attention(q, out, G, *many, scale)}
        if T == 1:
            routes["parent"] = routes["single"]     # (a one-token step never took the prefill kernel)
        for fn in routes.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        evs = {name: [] for name in routes}
        for _ in range(max(a.reps, 5)):
            for name, fn in routes.items():
                evs[name].append(timed(fn))
        torch.cuda.synchronize()
        ms = {name: sorted(x.elapsed_time(y) for x, y in e) for name, e in evs.items()}
        med = {name: t[len(t) // 2] for name, t in ms.items()}
        print(json.dumps({"case": f"bf16 step ctx={N} nf={nf} T={T}",
                          **{f"{name}_ms": {"median": round(med[name], 4), "min": round(t[0], 4), "max": round(t[-1], 4)}
                             for name, t in ms.items()},
                          "multi_over_single": round(med["multi"] / med["single"], 3),
                          "parent_over_multi": round(med["parent"] / med["multi"], 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["prefill", "decode", "decode_int4", "linear"])
    ap.add_argument("--rows", type=int, default=1, help="linear: token rows (batch size of the decode step)")
    ap.add_argument("--nf", type=int, default=4)
    ap.add_argument("--past", type=int, default=65536)
    ap.add_argument("--chunk", type=int, default=16384)
    ap.add_argument("--ctx", type=int, default=131072)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--flags", type=int, default=0)
    ap.add_argument("--uniform-nf", type=int, default=-1, help="decode: every layer has this many retrieval kv heads")
    ap.add_argument("--q-len", type=int, nargs="+", default=None,
                    help="decode / decode_int4: time a step of T tokens (one layer, --nf retrieval kv heads, --ctx rows) three ways")
    a = ap.parse_args()
    from duo_attn import _hip
    from duo_attn.backend import get_backend

    be = get_backend()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    G = HQ // HKV
    if a.what == "linear":
        # the four token-row linears of a Llama-3-8B decoder layer's decode step (csrc/duo_linear.hip) against the same
        # modules through torch (hipBLASLt GEMM at M = rows + separate norm / activation / add kernels); 32 distinct
        # weight sets so that nothing is served from L2 / MALL
        import torch.nn.functional as F
        Hd, I, L = 4096, 14336, 32
        rn = lambda *s_: (torch.randn(*s_, generator=g, device=dev, dtype=torch.float32) * 0.02).to(torch.bfloat16)
        Ws = [dict(q=rn(4096, Hd), k=rn(1024, Hd), v=rn(1024, Hd), o=rn(Hd, 4096), g=rn(I, Hd), u=rn(I, Hd), d=rn(Hd, I),
                   n1=rn(Hd).abs() + 1, n2=rn(Hd).abs() + 1) for _ in range(L)]
        x = rn(a.rows, Hd) * 50
        ao = rn(a.rows, 4096) * 50
        cases = {
            "qkv (rmsnorm prologue)": (lambda w: be.token_linear(x, [(w["q"], None), (w["k"], None), (w["v"], None)], norm=(w["n1"], 1e-5)),
                                       lambda w: [F.linear(be.rmsnorm(x, w["n1"], 1e-5), w[n]) for n in "qkv"], 6144 * Hd),
            "o_proj + residual": (lambda w: be.token_linear(ao, [(w["o"], None)], residual=x),
                                  lambda w: x + F.linear(ao, w["o"]), Hd * 4096),
            "gate|up (rmsnorm prologue)": (lambda w: be.token_linear(x, [(w["g"], None), (w["u"], None)], norm=(w["n2"], 1e-5)),
                                           lambda w: [F.linear(be.rmsnorm(x, w["n2"], 1e-5), w[n]) for n in "gu"], 2 * I * Hd),
        }
        gu = be.token_linear(x, [(Ws[0]["g"], None), (Ws[0]["u"], None)], norm=(Ws[0]["n2"], 1e-5))
        cases["down_proj (silu*mul prologue) + residual"] = (
            lambda w: be.token_linear(gu[:, :I], [(w["d"], None)], x2=gu[:, I:], residual=x),
            lambda w: x + F.linear(F.silu(gu[:, :I]) * gu[:, I:], w["d"]), Hd * I)
        tot = {"hip": 0.0, "torch": 0.0}
        for name, (hip_fn, torch_fn, nelem) in cases.items():
            res = {}
            for tag, fn in (("hip", hip_fn), ("torch", torch_fn)):
                avg, mn, med = time_it(lambda: [fn(w) for w in Ws], a.reps)
                res[tag] = avg / L * 1e3
                tot[tag] += avg / L * 1e3
            print(json.dumps({"case": f"{name} rows={a.rows}", "weight_MB": nelem * 2 / 1e6, "hip_us": round(res["hip"], 2),
                              "torch_us": round(res["torch"], 2), "hip_TBps": round(nelem * 2 / res["hip"] / 1e6, 3),
                              "torch_TBps": round(nelem * 2 / res["torch"] / 1e6, 3)}))
        wbytes = (6144 * Hd + Hd * 4096 + 3 * I * Hd) * 2
        print(json.dumps({"case": f"layer total rows={a.rows}", "hip_us": round(tot["hip"], 1), "torch_us": round(tot["torch"], 1),
                          "hip_TBps": round(wbytes / tot["hip"] / 1e6, 3), "torch_TBps": round(wbytes / tot["torch"] / 1e6, 3),
                          "x32_layers_ms": {k: round(v * 32 / 1e3, 3) for k, v in tot.items()}}))
        return
    scale = D ** -0.5
    if a.what == "prefill":
        nf, ns, S, past = a.nf, HKV - a.nf, a.chunk, a.past
        q = torch.randn(S, HQ, D, generator=g, device=dev).to(torch.bfloat16)
        kn, vn = pools(HKV, S, dev, g)
        out = torch.empty_like(q)
        fk, fv = pools(max(nf, 1), past + S, dev, g)
        sk, sv = pools(max(ns, 1), W, dev, g)
        full = (nf, 0, (fk[:past, :nf], fv[:past, :nf]), (fk[past:past + S, :nf], fv[past:past + S, :nf])) if nf else None
        stream = (ns, nf * G, (sk[:, :ns], sv[:, :ns]), (kn[:, nf:], vn[:, nf:])) if ns else None
        _hip.set_debug_flags(a.flags)
        avg, mn, med = time_it(lambda: be.attention(q, out, G, full, stream, scale), a.reps)
        tri = S * (S + 1) / 2
        flops = 4 * D * G * (nf * (S * past + tri) + ns * (S * min(past, W) + tri))
        print(json.dumps({"case": f"prefill nf={nf} past={past} S={S}", "avg_ms": avg, "min_ms": mn,
                          "tflops_avg": flops / avg / 1e9, "tflops_best": flops / mn / 1e9}))
    elif a.what == "decode_int4" and a.q_len:
        int4_multi_token(a, dev, g)
    elif a.what == "decode" and a.q_len:
        bf16_multi_token(a, be, dev, g)
    elif a.what == "decode_int4":
        import bench

        counts = bench.LLAMA3_8B_FULL_KV_HEADS
        N = a.ctx
        q = torch.randn(HQ, D, generator=g, device=dev).to(torch.float16)
        out = torch.empty_like(q)
        layers = []
        for nf in counts:
            ns = HKV - nf
            mk = lambda h, T: (torch.randint(0, 256, (h, T, 64), generator=g, device=dev, dtype=torch.uint8).permute(1, 0, 2),
                               (torch.rand(h, T, 2, generator=g, device=dev) * 0.3 + 0.01).to(torch.float16).permute(1, 0, 2))
            fkq, fksz = mk(max(nf, 1), N + 1)
            fvq, fvsz = mk(max(nf, 1), N + 1)
            skq, sksz = mk(max(ns, 1), W + 1)
            svq, svsz = mk(max(ns, 1), W + 1)
            full = _hip.make_int4_pool(fkq[:, :nf], fksz[:, :nf], fvq[:, :nf], fvsz[:, :nf], N + 1, 0) if nf else None
            stream = _hip.make_int4_pool(skq[:, :ns], sksz[:, :ns], svq[:, :ns], svsz[:, :ns], W + 1, nf * G) if ns else None
            layers.append((full, stream, (fkq, fksz, fvq, fvsz, skq, sksz, svq, svsz)))

        _hip.set_debug_flags(a.flags)

        def step():
            for full, stream, _ in layers:
                _hip.attn_decode_int4(q, out, G, full, stream, scale)

        avg, mn, med = time_it(step, a.reps)
        rows = sum(nf * (N + 1) + (HKV - nf) * (W + 1) for nf in counts)
        nbytes = rows * 2 * 68
        print(json.dumps({"case": f"int4 decode (split+merge) x32 layers ctx={N}", "avg_ms": avg, "min_ms": mn,
                          "GBps_avg": nbytes / avg / 1e6, "rows_per_us": rows / avg / 1e3,
                          "bf16_equivalent_GBps": rows * 512 / avg / 1e6}))
    else:
        import bench

        counts = bench.LLAMA3_8B_FULL_KV_HEADS if a.uniform_nf < 0 else [a.uniform_nf] * 8
        N = a.ctx
        q = torch.randn(1, HQ, D, generator=g, device=dev).to(torch.bfloat16)
        kn, vn = pools(HKV, 1, dev, g)
        out = torch.empty_like(q)
        layers = []
        for nf in counts:
            ns = HKV - nf
            fk, fv = pools(max(nf, 1), N + 1, dev, g)
            sk, sv = pools(max(ns, 1), W, dev, g)
            full = (nf, 0, (fk[:N, :nf], fv[:N, :nf]), (fk[N:N + 1, :nf], fv[N:N + 1, :nf])) if nf else None
            stream = (ns, nf * G, (sk[:, :ns], sv[:, :ns]), (kn[:, nf:], vn[:, nf:])) if ns else None
            layers.append((full, stream))
        _hip.set_debug_flags(a.flags | 2)

        def step():
            for full, stream in layers:
                be.attention(q, out, G, full, stream, scale)

        avg, mn, med = time_it(step, a.reps)
        nbytes = sum(bench.decode_bytes(counts, N))
        print(json.dumps({"case": f"decode split kernel x{len(counts)} layers ctx={N}" + (f" nf={a.uniform_nf}" if a.uniform_nf >= 0 else ""), "avg_ms": avg, "min_ms": mn,
                          "GBps_avg": nbytes / avg / 1e6, "GBps_best": nbytes / mn / 1e6,
                          "frac_of_8TBps": nbytes / avg / 1e6 / 8000}))
        _hip.set_debug_flags(0)


if __name__ == "__main__":
    main()
