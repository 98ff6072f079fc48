"""Test-side restatements for retrieval-head training (independent of the package's kernels).

* ``lambda_mask``: the Λ mask as the issue pins it (token mode = reference streaming_attn.py:14-24; block mode =
  Block-Sparse-Attention's streaming mask, restated: 128-row blocks, ``nsb`` sink blocks, ``nlb`` local blocks including
  the diagonal one).
* ``dense_attention`` / ``fa2_reference``: dense masked attention in any float type, and the FA2 arithmetic of the
  backward (P and dS rounded to bf16 where the kernel rounds them) — the "reference arithmetic" the GPU bars compare to.
* ``DenseLambdaBackend``: a backend whose Λ op is the dense torch computation, for the CPU plumbing tests.
* ``model_two_way_hidden``: the two-way decoder forward of a HF Llama (weights read from the model), restated in torch,
  used as the fp64 truth and the bf16 reference arithmetic of the model-level gate test.
"""
import math

import torch

BLOCK = 128


def lambda_mask(S, sink, recent, block_mode, device="cpu"):
    """bool [S, S]: row i sees key j.  block_mode 0: sink / recent in tokens; 1: in 128-row blocks."""
    i = torch.arange(S, device=device).view(S, 1)
    j = torch.arange(S, device=device).view(1, S)
    if block_mode:
        vis = (j // BLOCK < sink) | (i // BLOCK - j // BLOCK < recent)
    else:
        vis = (j < sink) | (j > i - recent)
    return vis & (j <= i)


def _expand(k, G):
    return k.repeat_interleave(G, dim=2)


def dense_attention(q, k, v, mask, dtype=torch.float32, round_p=False):
    """q [B, S, Hq, D], k / v [B, S, Hkv, D], mask [S, S] -> (out [B, S, Hq, D] in ``dtype``, lse [B, Hq, S]).
    round_p: P (relative to the row's true maximum, normalised) rounded to bf16 before P.V."""
    G = q.shape[2] // k.shape[2]
    qd, kd, vd = q.to(dtype), _expand(k, G).to(dtype), _expand(v, G).to(dtype)
    s = torch.einsum("bihd,bjhd->bhij", qd, kd) * (q.shape[-1] ** -0.5)
    s = s.masked_fill(~mask, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    if round_p:
        p = p.to(torch.bfloat16).to(dtype)
    out = torch.einsum("bhij,bjhd->bihd", p, vd)
    return out, lse


def attention_budget(q, k, v, mask):
    """sum_j p_j |v_j| (fp32): the P-rounding term of helpers.attn_close"""
    G = q.shape[2] // k.shape[2]
    s = torch.einsum("bihd,bjhd->bhij", q.float(), _expand(k, G).float()) * (q.shape[-1] ** -0.5)
    p = torch.softmax(s.masked_fill(~mask, float("-inf")), dim=-1)
    return torch.einsum("bhij,bjhd->bihd", p, _expand(v, G).float().abs())


def dense_grads(q, k, v, dout, mask, dtype=torch.float64):
    """autograd of the dense masked attention in ``dtype`` on the given (bf16) inputs: (dq, dk, dv) in ``dtype``"""
    with torch.enable_grad():           # (also when called from an autograd Function's backward)
        qd, kd, vd = (t.detach().to(dtype).requires_grad_(True) for t in (q, k, v))
        out, _ = dense_attention(qd, kd, vd, mask, dtype=dtype)
        out.backward(dout.to(dtype))
    return qd.grad, kd.grad, vd.grad


def fa2_reference(q, k, v, dout, mask):
    """The FA2 backward arithmetic in fp32 on the same bf16 inputs: P from the fp32 LSE, delta = rowsum(dO o O) with O the
    bf16 output, dS = P o (dP - delta) in fp32, P and dS rounded to bf16 before their products, GQA sums in fp32, outputs
    rounded to bf16.  Returns (dq, dk, dv) bf16."""
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    G = Hq // Hkv
    scale = D ** -0.5
    qf, kf, vf, df = q.float(), _expand(k, G).float(), _expand(v, G).float(), dout.float()
    s = torch.einsum("bihd,bjhd->bhij", qf, kf) * scale
    s = s.masked_fill(~mask, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    pb = p.to(torch.bfloat16).float()
    o = torch.einsum("bhij,bjhd->bihd", pb, vf).to(torch.bfloat16).float()
    dp = torch.einsum("bihd,bjhd->bhij", df, vf)
    delta = (df * o).sum(-1).transpose(1, 2)                      # [B, Hq, S]
    ds = (p * (dp - delta[..., None])).to(torch.bfloat16).float()
    dq = torch.einsum("bhij,bjhd->bihd", ds, kf) * scale
    dk = torch.einsum("bhij,bihd->bjhd", ds, qf) * scale
    dv = torch.einsum("bhij,bihd->bjhd", pb, df)
    dk = dk.view(B, S, Hkv, G, D).sum(3)
    dv = dv.view(B, S, Hkv, G, D).sum(3)
    return dq.to(torch.bfloat16), dk.to(torch.bfloat16), dv.to(torch.bfloat16)


def rms(x):
    return float(x.double().pow(2).mean().sqrt())


class DenseLambdaBackend:
    """A test backend: the Λ op as dense torch autograd (any device / dtype), the full branch's causal attention dense too.
    Only what the training forward calls is implemented."""

    def attention(self, q, out, group, full, stream, scale):
        n_kv, _, _, (k, v) = full
        S = q.shape[0]
        mask = torch.ones(S, S, dtype=torch.bool, device=q.device).tril()
        o, _ = dense_attention(q[None], k[None], v[None], mask, dtype=torch.float32)
        out.copy_(o[0].to(out.dtype))

    def lambda_attn_fwd(self, q, k, v, sink, recent, block_mode, scale):
        mask = lambda_mask(q.shape[1], sink, recent, block_mode, q.device)
        out, lse = dense_attention(q, k, v, mask, dtype=torch.float32)
        return out.to(q.dtype), lse

    def lambda_attn_bwd(self, q, k, v, out, lse, dout, sink, recent, block_mode, scale):
        mask = lambda_mask(q.shape[1], sink, recent, block_mode, q.device)
        dq, dk, dv = dense_grads(q, k, v, dout, mask, dtype=torch.float32)
        return dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype)


# ---------------------------------------------------------------------------------------------------------------------
# model level: the two-way decoder forward restated (HF Llama arithmetic), in a chosen precision
# ---------------------------------------------------------------------------------------------------------------------
def _rms_norm(x, w, eps, dtype):
    xf = x.to(torch.float32) if dtype != torch.float64 else x
    var = xf.pow(2).mean(-1, keepdim=True)
    y = xf * torch.rsqrt(var + eps)
    return w.to(dtype) * y.to(dtype)


def _rope(x, pos, theta, dtype):
    """HF rotary: the cos / sin tables are DEFINED in fp32 (LlamaRotaryEmbedding computes inv_freq, the angles and their
    cos / sin in fp32 whatever the model dtype, then casts), so every precision of the restatement starts from those
    tables — an fp64 table is a different function (it moves bf16-rounded table entries by an ulp here and there)"""
    D = x.shape[-1]
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.int64).float() / D))
    ang = pos.float()[:, None] * inv[None]
    emb = torch.cat([ang, ang], dim=-1)
    cos, sin = emb.cos().to(dtype), emb.sin().to(dtype)
    x1, x2 = x[..., : D // 2], x[..., D // 2:]
    rot = torch.cat([-x2, x1], dim=-1)
    return x * cos[None, :, None, :] + rot * sin[None, :, None, :]


def _attn(q, k, v, mask, dtype, round_p):
    """q [B, S, Hq, D]: fp32 scores (fp64 when dtype is fp64), P rounded to bf16 when round_p, output in dtype"""
    acc = torch.float64 if dtype == torch.float64 else torch.float32
    G = q.shape[2] // k.shape[2]
    s = torch.einsum("bihd,bjhd->bhij", q.to(acc), _expand(k, G).to(acc)) * (q.shape[-1] ** -0.5)
    s = s.masked_fill(~mask, float("-inf"))
    p = torch.softmax(s, dim=-1)
    if round_p:
        p = p.to(torch.bfloat16).to(acc)
    return torch.einsum("bhij,bjhd->bihd", p, _expand(v, G).to(acc)).to(dtype)


def model_two_way_hidden(model, input_ids, gates, sink, recent, block_mode, dtype):
    """last hidden states [2B, S, H] of the two-way forward of a HF Llama ``model`` (LlamaForCausalLM), restated with the
    model's weights cast to ``dtype``.  ``gates``: list of per-layer [Hkv] tensors (autograd flows into them).
    fp64: exact softmax; bf16: fp32 scores, P rounded to bf16 (the project's flash convention)."""
    cfg = model.config
    Hq, Hkv = cfg.num_attention_heads, cfg.num_key_value_heads
    D = cfg.head_dim
    G = Hq // Hkv
    B, S = input_ids.shape
    ids = torch.cat([input_ids, input_ids], dim=0)
    pos = torch.arange(S)
    causal = torch.ones(S, S, dtype=torch.bool).tril()
    lam = lambda_mask(S, sink, recent, block_mode)
    round_p = dtype != torch.float64
    theta = getattr(cfg, "rope_theta", None) or cfg.rope_parameters["rope_theta"]
    W = lambda t: t.detach().to(dtype)
    h = model.model.embed_tokens.weight.detach().to(dtype)[ids]
    for li, layer in enumerate(model.model.layers):
        at = layer.self_attn
        x = _rms_norm(h, layer.input_layernorm.weight.detach(), cfg.rms_norm_eps, dtype)
        q = (x @ W(at.q_proj.weight).T).view(2 * B, S, Hq, D)
        k = (x @ W(at.k_proj.weight).T).view(2 * B, S, Hkv, D)
        v = (x @ W(at.v_proj.weight).T).view(2 * B, S, Hkv, D)
        q, k = _rope(q, pos, theta, dtype), _rope(k, pos, theta, dtype)
        with torch.no_grad():
            full = _attn(q[:B], k[:B], v[:B], causal, dtype, round_p)
        stream = _attn(q[B:], k[B:], v[B:], lam, dtype, round_p)
        a = gates[li].clamp(0, 1).to(dtype).view(Hkv, 1).expand(Hkv, G).reshape(1, 1, Hq, 1)
        blend = (1 - a) * stream + a * full
        o = torch.cat([full, blend], dim=0).reshape(2 * B, S, Hq * D) @ W(at.o_proj.weight).T
        h = h + o
        x = _rms_norm(h, layer.post_attention_layernorm.weight.detach(), cfg.rms_norm_eps, dtype)
        mlp = layer.mlp
        g = x @ W(mlp.gate_proj.weight).T
        u = x @ W(mlp.up_proj.weight).T
        h = h + (torch.nn.functional.silu(g) * u) @ W(mlp.down_proj.weight).T
    return _rms_norm(h, model.model.norm.weight.detach(), cfg.rms_norm_eps, dtype)


def distill_loss(hidden, B):
    """train.py:136-146 with every label kept (world size 1)"""
    a, b = hidden[:B].double() if hidden.dtype == torch.float64 else hidden[:B].float(), hidden[B:]
    b = b.double() if hidden.dtype == torch.float64 else b.float()
    n = a.shape[0] * a.shape[1]
    return (a - b).pow(2).mean(dim=-1).sum() / n


def make_llama(seed, layers=4, hidden=1024, heads=8, kv_heads=4, inter=2048, vocab=500, theta=5e5, eps=1e-5):
    """the model-level test's LlamaForCausalLM: linears N(0, 1/fan_in), embeddings N(0, 1), norm weights 1 + 0.1 N(0, 1)"""
    from transformers import LlamaConfig, LlamaForCausalLM

    cfg = LlamaConfig(vocab_size=vocab, hidden_size=hidden, intermediate_size=inter, num_hidden_layers=layers,
                      num_attention_heads=heads, num_key_value_heads=kv_heads, head_dim=128, rope_theta=theta, rms_norm_eps=eps,
                      max_position_embeddings=4096, tie_word_embeddings=False, attn_implementation="eager")
    torch.manual_seed(seed)
    m = LlamaForCausalLM(cfg)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if "norm" in name:
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
            elif "embed_tokens" in name:
                p.copy_(torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) / math.sqrt(p.shape[1]))
    return m.eval()
