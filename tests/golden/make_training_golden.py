#!/usr/bin/env python3
"""Golden vectors of retrieval-head training from the REFERENCE'S OWN CODE (read-only, ``make_golden.REF``).

Run where the reference is present (as make_golden.py):

    python tests/golden/make_training_golden.py      # rewrites tests/golden/training_*.npz

Shims as in make_golden.py (``install_shims``: flash_attn_func as SDPA with an explicit causal mask, fp32), plus
``block_sparse_attn.block_streaming_attn_func`` (CUDA only, not vendored) stubbed by a dense restatement of
Block-Sparse-Attention's documented streaming mask: with 128-row blocks, query row i sees key j iff j <= i and
(j // 128 < sink_blocks or i // 128 - j // 128 < local_blocks).  WORLD_SIZE = 1.

Recorded, in fp32 with autograd, through the reference's ``llama_duo_attention_forward_two_way`` (llama.py:41-143) on
one attention module (Hq 4, Hkv 2, D 128, model hidden 64; weights and inputs rounded to bf16 first, so a bf16 run
sees the same numbers):
  * training_token.npz: streaming_attn_sdpa + generate_streaming_mask (streaming_attn.py:14-43), sink 64 / recent 128;
  * training_block.npz: streaming_attn_blocksparse_flash_attn + generate_streaming_info_blocksparse_flash_attn
    (streaming_attn.py:70-108), 1 sink block / 1 local block (sink 64 / recent 128 rounded up, llama.py:450-462);
each: the weights, the 2B-row input, the attention output, d(full_attention_heads) and d(streaming-half input) under a
fixed upstream gradient.  S = 384 (rows past sink + recent, and a 128-block the block mask excludes).
  * training_masks.npz: generate_streaming_mask for a few (seq_len, sink, recent).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import install_shims  # noqa: E402

Hq, Hkv, D, HID, S, B = 4, 2, 128, 64, 384, 1
SINK, RECENT = 64, 128
THETA = 5e5
MASKS = [(16, 2, 4), (40, 3, 8), (64, 0, 5), (100, 10, 30), (130, 64, 128), (7, 1, 1)]


def block_streaming_attn_func(q, k, v, cu_q, cu_k, head_mask_type, streaming_info, max_q, max_k, p_dropout=0.0,
                              is_causal=True, **kw):
    """dense restatement of the block mode on unpadded [B * S, H, D] rows (every sequence max_q long)"""
    nh, nkv = q.shape[1], k.shape[1]
    info = streaming_info.view(-1, 2)
    out = torch.empty_like(q)
    i = torch.arange(max_q)[:, None]
    j = torch.arange(max_k)[None, :]
    for b in range(len(cu_q) - 1):
        qs, ks = slice(int(cu_q[b]), int(cu_q[b + 1])), slice(int(cu_k[b]), int(cu_k[b + 1]))
        for h in range(nh):
            nsb, nlb = int(info[h, 0]), int(info[h, 1])
            vis = (j <= i) & ((j // 128 < nsb) | (i // 128 - j // 128 < nlb))
            kh = h // (nh // nkv)
            s = q[qs, h].float() @ k[ks, kh].float().T * (q.shape[-1] ** -0.5)
            p = torch.softmax(s.masked_fill(~vis, float("-inf")), dim=-1)
            out[qs, h] = (p @ v[ks, kh].float()).to(q.dtype)
    return out


def reference_module(weights, gates, impl):
    from transformers import LlamaConfig
    from transformers.models.llama.modeling_llama import LlamaAttention, LlamaRotaryEmbedding

    import duo_attn.patch.llama as rl
    from duo_attn.patch import streaming_attn as rs

    cfg = LlamaConfig(hidden_size=HID, num_attention_heads=Hq, num_key_value_heads=Hkv, head_dim=D, rope_theta=THETA,
                      max_position_embeddings=4096, attn_implementation="eager")
    m = LlamaAttention(cfg, layer_idx=0).float()
    with torch.no_grad():
        for n in ("q_proj", "k_proj", "v_proj", "o_proj"):
            getattr(m, n).weight.copy_(weights[n])
    # the attributes transformers 4.45's LlamaAttention had and the reference reads
    m.num_heads, m.num_key_value_heads, m.head_dim = Hq, Hkv, D
    m.num_key_value_groups, m.hidden_size = Hq // Hkv, Hq * D
    m.rotary_emb = LlamaRotaryEmbedding(cfg)
    m.forward = types.MethodType(rl.llama_duo_attention_forward_two_way, m)
    # what enable_llama_duo_attention_training sets per module (llama.py:473-494), Ulysses off
    m.register_parameter("full_attention_heads", torch.nn.Parameter(gates.clone()))
    if impl == "sdpa":
        m.register_buffer("streaming_mask", rs.generate_streaming_mask(S, SINK, RECENT, "cpu"))
        m.streaming_attn_func = rs.streaming_attn_sdpa
    else:
        m.register_buffer("streaming_mask", rs.generate_streaming_info_blocksparse_flash_attn(
            (SINK + 127) // 128, (RECENT + 127) // 128, Hq, "cpu"))
        m.streaming_attn_func = rs.streaming_attn_blocksparse_flash_attn
    m.full_attn_func = sys.modules["flash_attn"].flash_attn_func
    return m


def main():
    install_shims()
    bsa = types.ModuleType("block_sparse_attn")
    bsa.block_streaming_attn_func = block_streaming_attn_func
    sys.modules["block_sparse_attn"] = bsa
    os.environ["WORLD_SIZE"] = "1"
    from duo_attn.patch import streaming_attn as rs

    g = torch.Generator().manual_seed(20260)
    bf = lambda t: t.to(torch.bfloat16).float()
    weights = {
        "q_proj": bf(torch.randn(Hq * D, HID, generator=g) / HID ** 0.5),
        "k_proj": bf(torch.randn(Hkv * D, HID, generator=g) / HID ** 0.5),
        "v_proj": bf(torch.randn(Hkv * D, HID, generator=g) / HID ** 0.5),
        "o_proj": bf(torch.randn(HID, Hq * D, generator=g) / (Hq * D) ** 0.5),
    }
    gates = bf(0.2 + 0.6 * torch.rand(Hkv, generator=g))
    h = bf(torch.randn(2 * B, S, HID, generator=g))
    dout = bf(torch.randn(2 * B, S, HID, generator=g))
    position_ids = torch.arange(S)[None]
    for impl, name in (("sdpa", "training_token.npz"), ("blocksparse", "training_block.npz")):
        m = reference_module(weights, gates, impl)
        h_full = h[:B].clone()
        h_str = h[B:].clone().requires_grad_(True)
        out, _, _ = m(torch.cat([h_full, h_str], dim=0), position_ids=position_ids)
        out.backward(dout)
        rec = {k: v.to(torch.bfloat16).view(torch.int16).numpy() for k, v in weights.items()}
        rec.update(gates=gates.numpy(), h=h.to(torch.bfloat16).view(torch.int16).numpy(),
                   dout=dout.to(torch.bfloat16).view(torch.int16).numpy(), out=out.detach().numpy(),
                   d_gates=m.full_attention_heads.grad.numpy(), d_h_stream=h_str.grad.numpy(),
                   dims=np.array([Hq, Hkv, D, HID, S, B, SINK, RECENT]), rope_theta=np.array(THETA),
                   mode=np.array(0 if impl == "sdpa" else 1))
        np.savez_compressed(os.path.join(HERE, name), **rec)
    masks = {}
    for n, sink, recent in MASKS:
        masks[f"mask_{n}_{sink}_{recent}"] = rs.generate_streaming_mask(n, sink, recent, "cpu").numpy()
    np.savez_compressed(os.path.join(HERE, "training_masks.npz"), **masks)


if __name__ == "__main__":
    main()
