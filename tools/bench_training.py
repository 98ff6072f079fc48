#!/usr/bin/env python3
"""Retrieval-head training on one MI355X: the Λ-mask attention op and a whole training step.

    python tools/bench_training.py --op            # op level: HIP Λ forward / backward vs torch SDPA with the dense mask
    python tools/bench_training.py --step          # step level: Llama-3-8B shape, S = 32 000, layers checkpointed
    python tools/bench_training.py --op --step --json out.json

Op level (Hq 32, Hkv 8, B 1, sink 128 / recent 256, token and block mode, S = 4K..32K): the HIP op
(duo_lambda_attn_fwd_bf16 / duo_lambda_attn_bwd_bf16) against what the parent commit offers for the same computation,
torch SDPA with the reference's dense bool mask and enable_gqa=True (streaming_attn.py:27-43; the block mode's mask built
the same way), forward + backward, in the same process: HIP events, warm-up, median of --reps runs.  Useful FLOPs:
4 B Hq D sum_i n_i forward (n_i = keys row i sees), 2.5x that backward, as a fraction of the 2.5 PF/s dense bf16 peak.

Step level: random-init bf16 Llama-3-8B shape (32 layers, hidden 4096, 32 / 8 heads, intermediate 14336), B 1, decoder
layers under torch.utils.checkpoint, duo_attn.train.train_step; time per step split into the full branch (the batched
prefill launch), the Λ forward, the Λ backward and the rest, and the peak memory.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "duo-attention_amd"))

import torch  # noqa: E402

PEAK = 2.5e15


def visible_per_row(S, sink, recent, block_mode):
    """n_i for every row (torch int64 [S]): |[0, min(sink_end, i + 1))| + |[max(sink_end, lo_i), i]|"""
    i = torch.arange(S, dtype=torch.int64)
    if block_mode:
        sink_end, lo = sink * 128, (i // 128 - recent + 1) * 128
    else:
        sink_end, lo = sink, i - recent + 1
    n_sink = torch.clamp(torch.minimum(torch.full_like(i, sink_end), i + 1), min=0)
    start = torch.maximum(torch.full_like(i, sink_end), lo.clamp(min=0))
    return n_sink + (i - start + 1).clamp(min=0)


def dense_mask(S, sink, recent, block_mode, device):
    i = torch.arange(S, device=device).view(S, 1)
    j = torch.arange(S, device=device).view(1, S)
    if block_mode:
        vis = (j // 128 < sink) | (i // 128 - j // 128 < recent)
    else:
        vis = (j < sink) | (j > i - recent)
    return (vis & (j <= i)).view(1, 1, S, S)


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def op_level(sizes, reps):
    from duo_attn import _hip

    Hq, Hkv, D, B = 32, 8, 128, 1
    rows = []
    for mode, (sink, recent) in ((0, (128, 256)), (1, (1, 2))):
        for S in sizes:
            g = torch.Generator(device="cuda").manual_seed(S)
            q = torch.randn(B, S, Hq, D, device="cuda", generator=g).to(torch.bfloat16)
            k = torch.randn(B, S, Hkv, D, device="cuda", generator=g).to(torch.bfloat16)
            v = torch.randn(B, S, Hkv, D, device="cuda", generator=g).to(torch.bfloat16)
            dout = torch.randn(B, S, Hq, D, device="cuda", generator=g).to(torch.bfloat16)
            out, lse = _hip.lambda_attn_fwd(q, k, v, sink, recent, mode, D ** -0.5)
            t_f = timed(lambda: _hip.lambda_attn_fwd(q, k, v, sink, recent, mode, D ** -0.5), reps)
            t_b = timed(lambda: _hip.lambda_attn_bwd(q, k, v, out, lse, dout, sink, recent, mode, D ** -0.5), reps)
            flops_f = 4.0 * B * Hq * D * float(visible_per_row(S, sink, recent, mode).sum())
            row = {"mode": "block" if mode else "token", "S": S, "hip_fwd_ms": t_f, "hip_bwd_ms": t_b,
                   "hip_fwd_bwd_ms": t_f + t_b, "useful_tflops_fwd": flops_f / t_f / 1e9,
                   "useful_tflops_bwd": 2.5 * flops_f / t_b / 1e9, "peak_fraction_fwd": flops_f / t_f * 1e3 / PEAK,
                   "peak_fraction_bwd": 2.5 * flops_f / t_b * 1e3 / PEAK}
            try:
                mask = dense_mask(S, sink, recent, mode, "cuda")
                qt, kt, vt = (t.transpose(1, 2).detach().requires_grad_(True) for t in (q, k, v))
                dt = dout.transpose(1, 2)

                def sdpa():
                    o = torch.nn.functional.scaled_dot_product_attention(qt, kt, vt, attn_mask=mask, enable_gqa=True)
                    o.backward(dt)
                    qt.grad = kt.grad = vt.grad = None

                row["sdpa_fwd_bwd_ms"] = timed(sdpa, reps)
                row["speedup"] = row["sdpa_fwd_bwd_ms"] / row["hip_fwd_bwd_ms"]
                del mask, qt, kt, vt
            except (torch.cuda.OutOfMemoryError, RuntimeError) as e:      # noqa: PERF203
                row["sdpa_fwd_bwd_ms"] = None
                row["sdpa_error"] = type(e).__name__ + ": " + str(e).split("\n")[0][:160]
            torch.cuda.empty_cache()
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def step_level(S, steps, layers):
    from transformers import LlamaConfig, LlamaForCausalLM
    from torch.utils.checkpoint import checkpoint

    from duo_attn import backend as be_mod
    from duo_attn.patch import enable_duo_attention_training, set_full_attention_heads
    from duo_attn.train import train_step

    cfg = LlamaConfig(vocab_size=128256, hidden_size=4096, intermediate_size=14336, num_hidden_layers=layers,
                      num_attention_heads=32, num_key_value_heads=8, head_dim=128, rope_theta=5e5, rms_norm_eps=1e-5,
                      max_position_embeddings=131072)
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = LlamaForCausalLM(cfg).to(torch.bfloat16)
    enable_duo_attention_training(model, 128, 256, S, streaming_attn_implementation="blocksparse")
    gen = torch.Generator().manual_seed(1)
    set_full_attention_heads(model, [0.2 + 0.6 * torch.rand(8, generator=gen) for _ in range(layers)])
    decoder = model.model
    for n, p in decoder.named_parameters():
        p.requires_grad = "full_attention_heads" in n
    for layer in decoder.layers:
        inner = layer.forward
        layer.forward = (lambda f: (lambda *a, **kw: checkpoint(f, *a, use_reentrant=False, **kw)))(inner)

    be = be_mod.get_backend()
    spans = {"full_branch": [], "lambda_fwd": [], "lambda_bwd": []}

    def wrap(name, attr):
        fn = getattr(be, attr)

        def timed_call(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **kw)
            e1.record()
            spans[name].append((e0, e1))
            return r

        setattr(be, attr, timed_call)

    wrap("full_branch", "attention_batched")
    wrap("lambda_fwd", "lambda_attn_fwd")
    wrap("lambda_bwd", "lambda_attn_bwd")

    ids = torch.randint(0, cfg.vocab_size, (1, S), generator=gen).cuda()
    labels = ids.clone()
    res = []
    for it in range(steps + 1):
        for v in spans.values():
            v.clear()
        torch.cuda.reset_peak_memory_stats()
        decoder.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.time()
        a.record()
        train_step(decoder, ids, labels, reg_weight=0.05)
        b.record()
        b.synchronize()
        total = a.elapsed_time(b)
        parts = {k: sum(e0.elapsed_time(e1) for e0, e1 in v) for k, v in spans.items()}
        row = {"step": it, "warmup": it == 0, "ms": total, "wall_s": time.time() - t0,
               "peak_mem_gib": torch.cuda.max_memory_allocated() / 2 ** 30,
               **{k + "_ms": x for k, x in parts.items()}, "rest_ms": total - sum(parts.values()),
               "calls": {k: len(v) for k, v in spans.items()}}
        print(json.dumps(row), flush=True)
        res.append(row)
    return {"S": S, "layers": layers, "steps": [r for r in res if not r["warmup"]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--op", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--sizes", default="4096,8192,16384,32768")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seq", type=int, default=32000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0)}
    if a.op:
        out["op"] = op_level([int(s) for s in a.sizes.split(",")], a.reps)
    if a.step:
        out["step"] = step_level(a.seq, a.steps, a.layers)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
