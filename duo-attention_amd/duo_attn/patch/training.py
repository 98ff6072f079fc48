"""Retrieval-head training: the two-way layer forward and its enabler (reference ``llama.py:41-143,437-501``).

The input batch is 2B rows.  Rows [0, B) are the FULL half: projections, HF rotary, causal attention (the batched
prefill launch, one head class, no cached segment) and o_proj, all under ``no_grad``.  Rows [B, 2B) are the STREAMING
half, with autograd: projections, rotary, Λ-mask attention (``streaming_attn.LambdaAttention``, HIP forward and
backward), then ``(1 - a) * stream + a * full`` with ``a = full_attention_heads.clamp(0, 1)`` per kv head, then o_proj.
The gates are an ``nn.Parameter`` [Hkv] per layer in the model dtype.
"""
import types

import torch
from torch import nn

from ..backend import get_backend
from .streaming_attn import (
    BLOCK,
    generate_streaming_info_blocksparse_flash_attn,
    generate_streaming_mask,
    lambda_attention,
)
from .tuple_kv_cache import enable_tuple_kv_cache_for_model, tuple_rotary

IMPLEMENTATIONS = ("blocksparse", "sdpa")


def duo_attention_forward_two_way(
    self,
    hidden_states,
    attention_mask=None,
    position_ids=None,
    past_key_value=None,
    output_attentions=False,
    use_cache=False,
    position_embeddings=None,
    **kwargs,
):
    bsz2, q_len, _ = hidden_states.size()
    if bsz2 % 2:
        raise ValueError(f"the two-way training forward takes a doubled batch (full rows, then streaming rows); got {bsz2}")
    bsz = bsz2 // 2
    cfg = self.config
    num_heads, num_kv = cfg.num_attention_heads, cfg.num_key_value_heads
    head_dim = getattr(self, "head_dim", cfg.hidden_size // num_heads)
    groups = num_heads // num_kv
    cos, sin = position_embeddings
    be = get_backend()

    with torch.no_grad():
        full_h = hidden_states[:bsz]
        fq = self.q_proj(full_h).view(bsz, q_len, num_heads, head_dim)
        fk = self.k_proj(full_h).view(bsz, q_len, num_kv, head_dim)
        fv = self.v_proj(full_h).view(bsz, q_len, num_kv, head_dim)
        fq, fk = tuple_rotary(fq, fk, cos, sin)
        full_out = torch.empty_like(fq)
        # every head full-causal over the sequence itself: the first chunk of the eval forward (_duo.py:618-623)
        if hasattr(be, "attention_batched"):
            be.attention_batched(fq, full_out, groups, (num_kv, 0, None, (fk, fv)), None, head_dim ** -0.5)
        else:
            for b in range(bsz):
                be.attention(fq[b], full_out[b], groups, (num_kv, 0, None, (fk[b], fv[b])), None, head_dim ** -0.5)

    str_h = hidden_states[bsz:]
    sq = self.q_proj(str_h).view(bsz, q_len, num_heads, head_dim)
    sk = self.k_proj(str_h).view(bsz, q_len, num_kv, head_dim)
    sv = self.v_proj(str_h).view(bsz, q_len, num_kv, head_dim)
    sq, sk = tuple_rotary(sq, sk, cos, sin)
    sink, recent, block_mode = self._duo_lambda
    stream_out = lambda_attention(sq, sk, sv, sink, recent, block_mode)

    a = self.full_attention_heads.clamp(0, 1).view(num_kv, 1).expand(num_kv, groups).reshape(1, 1, num_heads, 1)
    blend = (1 - a) * stream_out + a * full_out

    with torch.no_grad():
        full_o = self.o_proj(full_out.reshape(bsz, q_len, num_heads * head_dim))
    stream_o = self.o_proj(blend.reshape(bsz, q_len, num_heads * head_dim))
    return torch.cat([full_o, stream_o], dim=0), None, None


def _check_structure(model):
    """what the HIP training path covers, checked before anything is changed"""
    inner = getattr(model, "model", None)
    layers = getattr(inner, "layers", None)
    if layers is None or len(layers) == 0:
        raise NotImplementedError("retrieval-head training needs a HF causal LM with model.model.layers[*].self_attn")
    cfg = getattr(model, "config", None)
    for i, layer in enumerate(layers):
        attn = getattr(layer, "self_attn", None)
        if attn is None or not all(isinstance(getattr(attn, n, None), nn.Linear)
                                   for n in ("q_proj", "k_proj", "v_proj", "o_proj")):
            raise NotImplementedError(f"layer {i}: self_attn with q/k/v/o projections expected")
    num_heads, num_kv = cfg.num_attention_heads, cfg.num_key_value_heads
    head_dim = getattr(layers[0].self_attn, "head_dim", None) or getattr(cfg, "head_dim", None) or cfg.hidden_size // num_heads
    if head_dim != 128:
        raise NotImplementedError(f"head_dim {head_dim}: the HIP attention kernels cover head_dim 128 only")
    if num_heads % num_kv:
        raise NotImplementedError(f"{num_heads} q heads over {num_kv} kv heads")
    return num_heads, num_kv


def _check_ulysses(enable_ulysses_attention):
    if not enable_ulysses_attention:
        return
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError("sequence-parallel (Ulysses) training across more than one rank is not covered; "
                                  "on one rank it is the identity")


def enable_duo_attention_training(model, sink_size, recent_size, max_length, initial_value=1.0,
                                  enable_ulysses_attention=False, streaming_attn_implementation="blocksparse"):
    """reference llama.py:437-501 (llama and mistral alike).  ``sink_size`` / ``recent_size`` in tokens; the block mode
    ("blocksparse", the default) rounds both up to whole 128-row blocks once, here."""
    num_heads, num_kv = _check_structure(model)
    _check_ulysses(enable_ulysses_attention)
    if streaming_attn_implementation not in IMPLEMENTATIONS:
        raise ValueError(f"Unsupported streaming attention implementation: {streaming_attn_implementation}")
    sink_size, recent_size = int(sink_size), int(recent_size)
    if sink_size < 0 or recent_size < 0 or sink_size + recent_size < 1:
        raise ValueError(f"sink_size {sink_size} / recent_size {recent_size}: a row must see at least one key")

    enable_tuple_kv_cache_for_model(model)      # the tuple model forward, as the reference (llama.py:446)
    device = next(model.parameters()).device
    dtype = next(model.parameters()).dtype
    if streaming_attn_implementation == "blocksparse":
        sink_blocks = (sink_size + BLOCK - 1) // BLOCK
        local_blocks = (recent_size + BLOCK - 1) // BLOCK
        streaming_mask = generate_streaming_info_blocksparse_flash_attn(sink_blocks, local_blocks, num_heads, device)
        params = (sink_blocks, local_blocks, 1)
    else:
        streaming_mask = generate_streaming_mask(max_length, sink_size, recent_size, device)
        params = (sink_size, recent_size, 0)

    for layer in model.model.layers:
        module = layer.self_attn
        module.forward = types.MethodType(duo_attention_forward_two_way, module)
        module.sink_size = sink_size
        module.recent_size = recent_size
        module._duo_lambda = params
        module.register_parameter(
            "full_attention_heads",
            nn.Parameter(torch.ones(num_kv, device=device, dtype=dtype) * initial_value, requires_grad=True),
        )
        module.register_buffer("streaming_mask", streaming_mask)
