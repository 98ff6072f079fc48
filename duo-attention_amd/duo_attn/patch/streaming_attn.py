"""Streaming (Λ-mask) attention of retrieval-head training — the reference's public names
(``duo_attn/patch/streaming_attn.py:14-108``), each running on the HIP op ``duo_lambda_attn_{fwd,bwd}_bf16`` through
:class:`LambdaAttention` (forward and backward; no dense S x S mask is ever applied).

Query row i (0 = first token of the sequence) sees key j iff j <= i and
  * token mode (``streaming_attn_sdpa`` with ``generate_streaming_mask``): j < sink or j > i - recent;
  * block mode (``streaming_attn_blocksparse_flash_attn``): with 128-row blocks, j // 128 < sink_blocks or
    i // 128 - j // 128 < local_blocks (the local blocks include the diagonal block).
A key in both ranges is counted once.  The mask objects the two generators return carry their parameters as host
integers (``.duo_lambda``), so a call never reads them back from the device.
"""
import torch

from ..backend import get_backend

BLOCK = 128     # rows per block of the block mode


class LambdaAttention(torch.autograd.Function):
    """out = Λ-mask attention(q [B, S, Hq, D], k / v [B, S, Hkv, D]) with softmax scale 1 / sqrt(D); GQA by head groups.
    ``block_mode`` 0: ``sink`` / ``recent`` in tokens; 1: in 128-row blocks.  The backward is deterministic."""

    @staticmethod
    def forward(ctx, q, k, v, sink: int, recent: int, block_mode: int):
        scale = q.shape[-1] ** -0.5
        out, lse = get_backend().lambda_attn_fwd(q, k, v, sink, recent, block_mode, scale)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.params = (sink, recent, block_mode, scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        sink, recent, block_mode, scale = ctx.params
        dq, dk, dv = get_backend().lambda_attn_bwd(q, k, v, out, lse, dout, sink, recent, block_mode, scale)
        return dq, dk, dv, None, None, None


def lambda_attention(q, k, v, sink: int, recent: int, block_mode: int):
    return LambdaAttention.apply(q, k, v, int(sink), int(recent), int(block_mode))


@torch.no_grad()
def generate_streaming_mask(seq_len, sink_size, recent_size, device):
    """The token-mode mask as the reference builds it: bool [1, 1, N, N], N = seq_len rounded up to a multiple of 8,
    True where row i sees key j.  ``.duo_lambda`` = (sink_size, recent_size, 0)."""
    n = (seq_len + 7) // 8 * 8
    i = torch.arange(n).view(n, 1)
    j = torch.arange(n).view(1, n)
    mask = (j <= i) & ((j < sink_size) | (j > i - recent_size))
    mask = mask.to(device=device).view(1, 1, n, n)
    mask.duo_lambda = (int(sink_size), int(recent_size), 0)
    return mask


def _token_params(mask):
    p = getattr(mask, "duo_lambda", None)
    if p is not None:
        return p
    # a mask built elsewhere (or moved by Module.to, which drops the attribute): read its last row ONCE and cache it —
    # row n-1 sees a leading run of `sink` keys and a trailing run of `recent` keys (all of it: fully causal)
    last = mask[0, 0, -1].cpu()
    n = last.numel()
    if bool(last.all()):
        p = (0, n, 0)
    else:
        sink = int(torch.cumprod(last.int(), 0).sum())
        recent = int(torch.cumprod(last.flip(0).int(), 0).sum())
        p = (sink, recent, 0)
    mask.duo_lambda = p
    return p


def streaming_attn_sdpa(query_states, key_states, value_states, streaming_causal_mask):
    """reference ``streaming_attn_sdpa`` (SDPA with the dense mask, ``enable_gqa=True``): [B, S, H, D] in and out"""
    sink, recent, _ = _token_params(streaming_causal_mask)
    return lambda_attention(query_states, key_states, value_states, sink, recent, 0)


def generate_streaming_info_blocksparse_flash_attn(sink_block_num, local_block_num, n_query_heads, device):
    """The block mode's per-head ``[sink_block_num, local_block_num] * n_query_heads`` int32 tensor, as the reference
    builds it.  ``.duo_lambda`` = (sink_block_num, local_block_num, 1)."""
    info = torch.tensor([sink_block_num, local_block_num] * n_query_heads, device=device, dtype=torch.int32)
    info.duo_lambda = (int(sink_block_num), int(local_block_num), 1)
    return info


def _block_params(info):
    p = getattr(info, "duo_lambda", None)
    if p is None:
        head0 = info[:2].tolist()       # one read-back; every head carries the same pair
        p = (int(head0[0]), int(head0[1]), 1)
        info.duo_lambda = p
    return p


def streaming_attn_blocksparse_flash_attn(query_states, key_states, value_states, streaming_info):
    """reference ``streaming_attn_blocksparse_flash_attn`` (Block-Sparse-Attention's streaming mask, causal): [B, S, H, D]
    in and out"""
    sink_blocks, local_blocks, _ = _block_params(streaming_info)
    return lambda_attention(query_states, key_states, value_states, sink_blocks, local_blocks, 1)
