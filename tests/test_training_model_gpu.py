"""Retrieval-head training on the MI355X, above the op: the reference's own two-way module forward (fixtures), model-level
gate gradients against an fp64 restatement (tests/training_ref.py), activation checkpointing, the Λ op at full size,
and a train -> save -> load -> eval round trip.  Measured ratios go to helpers.PARITY_LOG."""
import copy
import json
import math
import os

import numpy as np
import pytest
import torch

from helpers import PARITY_LOG
from training_ref import _attn, _expand, distill_loss, lambda_mask, make_llama, model_two_way_hidden, rms

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def _freeze_all_but_gates(decoder):
    for n, p in decoder.named_parameters():
        p.requires_grad = "full_attention_heads" in n


# ---------------------------------------------------------------------------------------------------------------------
# 6. module golden: the reference's llama_duo_attention_forward_two_way (fp32, autograd) on one attention module
# ---------------------------------------------------------------------------------------------------------------------
def _fixture(name):
    d = np.load(os.path.join(HERE, "golden", name))
    bf = lambda k: torch.from_numpy(d[k].astype(np.int16)).view(torch.bfloat16)
    return d, bf


def _module_model(d, bf, device, dtype):
    from transformers import LlamaConfig, LlamaForCausalLM

    Hq, Hkv, D, HID = (int(x) for x in d["dims"][:4])
    cfg = LlamaConfig(vocab_size=16, hidden_size=HID, intermediate_size=64, num_hidden_layers=1, num_attention_heads=Hq,
                      num_key_value_heads=Hkv, head_dim=D, rope_theta=float(d["rope_theta"]), max_position_embeddings=4096)
    m = LlamaForCausalLM(cfg).to(device=device, dtype=dtype)
    with torch.no_grad():
        for n in ("q_proj", "k_proj", "v_proj", "o_proj"):
            getattr(m.model.layers[0].self_attn, n).weight.copy_(bf(n).to(dtype))
    return m


def _restated_module(m, h, gates, sink, recent, mode):
    """the test-local restatement of the two-way module forward in the model's dtype (bf16: fp32 scores, P rounded)"""
    at = m.model.layers[0].self_attn
    cfg = m.config
    Hq, Hkv, D = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
    B2, S, _ = h.shape
    B = B2 // 2
    cos, sin = m.model.rotary_emb(h, torch.arange(S)[None])
    dtype = h.dtype

    def proj(x):
        q = at.q_proj(x).view(x.shape[0], S, Hq, D)
        k = at.k_proj(x).view(x.shape[0], S, Hkv, D)
        v = at.v_proj(x).view(x.shape[0], S, Hkv, D)
        rot = lambda t: torch.cat([-t[..., D // 2:], t[..., : D // 2]], dim=-1)
        c, s = cos[:, :, None, :], sin[:, :, None, :]
        return q * c + rot(q) * s, k * c + rot(k) * s, v

    with torch.no_grad():
        q, k, v = proj(h[:B])
        full = _attn(q, k, v, torch.ones(S, S, dtype=torch.bool).tril(), dtype, True)
    q, k, v = proj(h[B:])
    stream = _attn(q, k, v, lambda_mask(S, sink, recent, mode), dtype, True)
    a = gates.clamp(0, 1).view(Hkv, 1).expand(Hkv, Hq // Hkv).reshape(1, 1, Hq, 1)
    blend = (1 - a) * stream + a * full
    with torch.no_grad():
        fo = at.o_proj(full.reshape(B, S, Hq * D))
    return torch.cat([fo, at.o_proj(blend.reshape(B, S, Hq * D))], dim=0)


@pytest.mark.parametrize("name", ["training_token.npz", "training_block.npz"])
def test_module_golden(name):
    from duo_attn.patch import enable_duo_attention_training

    d, bf = _fixture(name)
    Hq, Hkv, D, HID, S, B, SINK, RECENT = (int(x) for x in d["dims"])
    mode = int(d["mode"])
    impl = "blocksparse" if mode else "sdpa"
    ps, pr = ((SINK + 127) // 128, (RECENT + 127) // 128) if mode else (SINK, RECENT)
    want = {"out": torch.from_numpy(d["out"]), "d_gates": torch.from_numpy(d["d_gates"]),
            "d_h_stream": torch.from_numpy(d["d_h_stream"])}

    # the bar: a bf16 CPU run of the restatement against the fixture
    m = _module_model(d, bf, "cpu", torch.bfloat16)
    gates = torch.from_numpy(d["gates"]).to(torch.bfloat16).requires_grad_(True)
    h = bf("h")
    h_str = h[B:].clone().requires_grad_(True)
    out = _restated_module(m, torch.cat([h[:B], h_str]), gates, ps, pr, mode)
    out.backward(bf("dout"))
    ref_err = {"out": _rel(out, want["out"]), "d_gates": _rel(gates.grad, want["d_gates"]),
               "d_h_stream": _rel(h_str.grad, want["d_h_stream"])}

    m = _module_model(d, bf, "cuda", torch.bfloat16)
    enable_duo_attention_training(m, SINK, RECENT, S, streaming_attn_implementation=impl)
    at = m.model.layers[0].self_attn
    with torch.no_grad():
        at.full_attention_heads.copy_(torch.from_numpy(d["gates"]).to(torch.bfloat16))
    h = bf("h").cuda()
    h_str = h[B:].clone().requires_grad_(True)
    x = torch.cat([h[:B], h_str])
    pe = m.model.rotary_emb(x, torch.arange(S, device="cuda")[None])
    out, _, _ = at(hidden_states=x, position_embeddings=pe)
    out.backward(bf("dout").cuda())
    got = {"out": _rel(out, want["out"]), "d_gates": _rel(at.full_attention_heads.grad, want["d_gates"]),
           "d_h_stream": _rel(h_str.grad, want["d_h_stream"])}
    for k in got:
        PARITY_LOG[f"model: training module golden {name} {k}"] = {
            "rel_l2": got[k], "rel_l2_bf16_restatement": ref_err[k], "ratio": got[k] / ref_err[k], "bar": 2.0}
    for k in got:
        assert got[k] <= 2 * ref_err[k], f"{name} {k}: rel L2 {got[k]:.3e} > 2 x bf16 restatement's {ref_err[k]:.3e}"


# ---------------------------------------------------------------------------------------------------------------------
# 7. model-level gate gradients
# ---------------------------------------------------------------------------------------------------------------------
def _gates_for(seed, L=4, Hkv=4):
    g = torch.Generator().manual_seed(100 + seed)
    return [0.2 + 0.6 * torch.rand(Hkv, generator=g) for _ in range(L)]


def _hip_model_grads(model_cpu, ids, gates, sink, recent, impl, checkpoint=False):
    from duo_attn.patch import enable_duo_attention_training, get_full_attention_heads, set_full_attention_heads

    m = copy.deepcopy(model_cpu).to(device="cuda", dtype=torch.bfloat16)
    enable_duo_attention_training(m, sink, recent, ids.shape[1], streaming_attn_implementation=impl)
    set_full_attention_heads(m, [g.clone() for g in gates])
    decoder = m.model
    _freeze_all_but_gates(decoder)
    if checkpoint:
        from torch.utils.checkpoint import checkpoint as ckpt

        for layer in decoder.layers:
            inner = layer.forward
            layer.forward = (lambda f: (lambda *a, **kw: ckpt(f, *a, use_reentrant=False, **kw)))(inner)
    S = ids.shape[1]
    out = decoder(input_ids=torch.cat([ids, ids]).cuda(), position_ids=torch.arange(S, device="cuda")[None])[0]
    loss = distill_loss(out, ids.shape[0])
    loss.backward()
    return loss.detach().double().cpu(), torch.cat([h.grad.detach().double().cpu() for h in get_full_attention_heads(m)])


def _restated_grads(model_cpu, ids, gates, ps, pr, mode, dtype):
    g = [x.to(dtype).requires_grad_(True) for x in gates]
    h = model_two_way_hidden(model_cpu, ids, g, ps, pr, mode, dtype)
    loss = distill_loss(h, ids.shape[0])
    loss.backward()
    return loss.detach().double(), torch.cat([x.grad.double() for x in g])


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("impl,S", [("sdpa", 512), ("blocksparse", 768)])
def test_model_gate_gradients(impl, S, seed):
    sink, recent = 64, 128
    mode = 1 if impl == "blocksparse" else 0
    ps, pr = ((sink + 127) // 128, (recent + 127) // 128) if mode else (sink, recent)
    model = make_llama(seed)
    ids = torch.randint(0, 500, (1, S), generator=torch.Generator().manual_seed(seed))
    gates = _gates_for(seed)
    l64, g64 = _restated_grads(model, ids, gates, ps, pr, mode, torch.float64)
    l16, g16 = _restated_grads(model, ids, gates, ps, pr, mode, torch.bfloat16)
    lh, gh = _hip_model_grads(model, ids, gates, sink, recent, impl)
    e_loss16, e_loss = abs(float(l16 - l64)) / abs(float(l64)), abs(float(lh - l64)) / abs(float(l64))
    e_g16, e_g = float((g16 - g64).norm() / g64.norm()), float((gh - g64).norm() / g64.norm())
    trusted = g64.abs() > 3 * (g16 - g64).abs()
    flips = int(((torch.sign(gh) != torch.sign(g64)) & trusted).sum())
    what = f"model: training gates {impl} S{S} seed{seed}"
    PARITY_LOG[what] = {"loss_rel_err": e_loss, "loss_rel_err_bf16_restatement": e_loss16,
                        "gate_grad_rel_l2": e_g, "gate_grad_rel_l2_bf16_restatement": e_g16,
                        "gate_grad_ratio": e_g / e_g16, "loss_ratio": e_loss / e_loss16 if e_loss16 > 0 else 0.0,
                        "excluded_gates": int((~trusted).sum()), "sign_flips": flips, "bar": 2.0}
    assert e_loss <= 2 * e_loss16, f"{what}: loss rel err {e_loss:.3e} > 2 x bf16 restatement's {e_loss16:.3e}"
    assert e_g <= 2 * e_g16, f"{what}: gate-gradient rel L2 {e_g:.3e} > 2 x bf16 restatement's {e_g16:.3e}"
    assert flips == 0, f"{what}: {flips} gate gradients with the wrong sign"
    assert int((~trusted).sum()) <= g64.numel() // 8


# ---------------------------------------------------------------------------------------------------------------------
# 5. checkpointed and plain gate gradients are bitwise equal
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", ["sdpa", "blocksparse"])
def test_checkpointed_gate_gradients_are_bitwise_equal(impl):
    model = make_llama(5)
    ids = torch.randint(0, 500, (1, 700), generator=torch.Generator().manual_seed(5))
    gates = _gates_for(5)
    l0, g0 = _hip_model_grads(model, ids, gates, 64, 128, impl)
    l1, g1 = _hip_model_grads(model, ids, gates, 64, 128, impl, checkpoint=True)
    l2, g2 = _hip_model_grads(model, ids, gates, 64, 128, impl)
    assert torch.equal(g0, g2) and torch.equal(l0, l2)            # a rerun
    assert torch.equal(g0, g1) and torch.equal(l0, l1)            # a recompute under checkpointing
    assert bool((g0 != 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# 4. full size: Hq 32, Hkv 8, S 32 768, block mode 128 / 256, on sampled rows and keys
# ---------------------------------------------------------------------------------------------------------------------
def test_full_size_sampled():
    from duo_attn import _hip

    S, Hq, Hkv, D = 32768, 32, 8, 128
    G = Hq // Hkv
    nsb, nlb = 1, 2                              # sink 128 / recent 256 in 128-row blocks
    g = torch.Generator(device="cuda").manual_seed(11)
    q = torch.randn(1, S, Hq, D, device="cuda", generator=g).to(torch.bfloat16)
    k = torch.randn(1, S, Hkv, D, device="cuda", generator=g).to(torch.bfloat16)
    v = torch.randn(1, S, Hkv, D, device="cuda", generator=g).to(torch.bfloat16)
    dout = torch.randn(1, S, Hq, D, device="cuda", generator=g).to(torch.bfloat16)
    out, lse = _hip.lambda_attn_fwd(q, k, v, nsb, nlb, 1, D ** -0.5)
    dq, dk, dv = _hip.lambda_attn_bwd(q, k, v, out, lse, dout, nsb, nlb, 1, D ** -0.5)
    torch.cuda.synchronize()

    # sampled query rows: every 128-block edge +-1, the first and last rows
    edges = torch.arange(0, S + 1, 128)
    rows = torch.unique(torch.cat([edges - 1, edges, edges + 1, torch.tensor([0, S - 1])]).clamp(0, S - 1)).cuda()
    # rows i see keys [0, 128) and [128 (i // 128 - 1), i]: gather those keys per row (a block-diagonal dense slab)
    errs = {"out": [], "out_ref": [], "dq": [], "dq_ref": []}
    for chunk in rows.split(64):
        lo = ((chunk.min() // 128 - 1).clamp(min=0) * 128).item()
        hi = int(chunk.max()) + 1
        keys = torch.unique(torch.cat([torch.arange(0, 128, device="cuda"), torch.arange(lo, hi, device="cuda")]))
        mask = ((keys[None, :] // 128 < nsb) | (chunk[:, None] // 128 - keys[None, :] // 128 < nlb)) & (keys[None, :] <= chunk[:, None])
        qs, ks, vs, ds = q[:, chunk], k[:, keys], v[:, keys], dout[:, chunk]
        # dense on the gathered (row, key) slab: exact fp64, and the fp32 / bf16-P reference arithmetic
        s64 = torch.einsum("bihd,bjhd->bhij", qs.double(), _expand(ks, G).double()) * D ** -0.5
        s64 = s64.masked_fill(~mask, float("-inf"))
        p64 = torch.softmax(s64, -1)
        o64 = torch.einsum("bhij,bjhd->bihd", p64, _expand(vs, G).double())
        s32 = (torch.einsum("bihd,bjhd->bhij", qs.float(), _expand(ks, G).float()) * D ** -0.5).masked_fill(~mask, float("-inf"))
        p32 = torch.softmax(s32, -1)
        o_ref = torch.einsum("bhij,bjhd->bihd", p32.to(torch.bfloat16).float(), _expand(vs, G).float()).to(torch.bfloat16)
        errs["out"].append((out[:, chunk].double() - o64).flatten())
        errs["out_ref"].append((o_ref.double() - o64).flatten())
        # dQ of these rows: dS over the same slab (delta from the kernel-independent bf16-P output)
        dp64 = torch.einsum("bihd,bjhd->bhij", ds.double(), _expand(vs, G).double())
        delta64 = (ds.double() * o64).sum(-1).transpose(1, 2)
        dq64 = torch.einsum("bhij,bjhd->bihd", p64 * (dp64 - delta64[..., None]), _expand(ks, G).double()) * D ** -0.5
        dp32 = torch.einsum("bihd,bjhd->bhij", ds.float(), _expand(vs, G).float())
        delta32 = (ds.float() * o_ref.float()).sum(-1).transpose(1, 2)
        ds32 = (p32 * (dp32 - delta32[..., None])).to(torch.bfloat16).float()
        dq_ref = (torch.einsum("bhij,bjhd->bihd", ds32, _expand(ks, G).float()) * D ** -0.5).to(torch.bfloat16)
        errs["dq"].append((dq[:, chunk].double() - dq64).flatten())
        errs["dq_ref"].append((dq_ref.double() - dq64).flatten())
    for name in ("out", "dq"):
        e, r = rms(torch.cat(errs[name])), rms(torch.cat(errs[name + "_ref"]))
        bar = 1.12 + 3 / math.sqrt(torch.cat(errs[name]).numel()) if name == "out" else 1.25
        PARITY_LOG[f"lambda full size S{S} {name}"] = {"rms_err": e, "rms_err_reference_arithmetic": r, "ratio": e / r,
                                                       "bar": bar}
        assert e <= bar * r, f"full size {name}: rms err {e:.3e} > {bar:.3f} x reference arithmetic's {r:.3e}"

    # sampled keys: every sink key and a few band keys; dK / dV over every row that sees them (chunked fp64 on the GPU)
    keys = torch.cat([torch.arange(0, 128), torch.tensor([128, 129, 255, 256, 4095, 4096, 20000, S - 2, S - 1])]).cuda()
    acc = {n: torch.zeros(keys.numel(), Hkv, D, dtype=torch.float64, device="cuda") for n in ("dk", "dv", "dk_r", "dv_r")}
    for r0 in range(0, S, 2048):
        ri = torch.arange(r0, min(S, r0 + 2048), device="cuda")
        mask = ((keys[None, :] // 128 < nsb) | (ri[:, None] // 128 - keys[None, :] // 128 < nlb)) & (keys[None, :] <= ri[:, None])
        if not bool(mask.any()):
            continue
        # softmax statistics of these rows come from their own full key sets: the kernel-independent LSE of each row
        lo = max(0, (r0 // 128 - 1) * 128)
        kall = torch.unique(torch.cat([torch.arange(0, 128, device="cuda"), torch.arange(lo, int(ri[-1]) + 1, device="cuda")]))
        mall = ((kall[None, :] // 128 < nsb) | (ri[:, None] // 128 - kall[None, :] // 128 < nlb)) & (kall[None, :] <= ri[:, None])
        qs, ds = q[:, ri], dout[:, ri]
        sa = (torch.einsum("bihd,bjhd->bhij", qs.double(), _expand(k[:, kall], G).double()) * D ** -0.5).masked_fill(~mall, float("-inf"))
        lse64 = torch.logsumexp(sa, -1)
        pa = torch.exp(sa - lse64[..., None])
        o64 = torch.einsum("bhij,bjhd->bihd", pa, _expand(v[:, kall], G).double())
        sa32 = (torch.einsum("bihd,bjhd->bhij", qs.float(), _expand(k[:, kall], G).float()) * D ** -0.5).masked_fill(~mall, float("-inf"))
        lse32 = torch.logsumexp(sa32, -1)
        o32 = torch.einsum("bhij,bjhd->bihd", torch.exp(sa32 - lse32[..., None]).to(torch.bfloat16).float(),
                           _expand(v[:, kall], G).float()).to(torch.bfloat16).float()
        del sa, pa, sa32
        s = (torch.einsum("bihd,bjhd->bhij", qs.double(), _expand(k[:, keys], G).double()) * D ** -0.5).masked_fill(~mask, float("-inf"))
        p = torch.exp(s - lse64[..., None])
        dp = torch.einsum("bihd,bjhd->bhij", ds.double(), _expand(v[:, keys], G).double())
        dS = p * (dp - (ds.double() * o64).sum(-1).transpose(1, 2)[..., None])
        acc["dv"] += torch.einsum("bhij,bihd->bjhd", p, ds.double())[0].view(-1, Hkv, G, D).sum(2)
        acc["dk"] += (torch.einsum("bhij,bihd->bjhd", dS, qs.double()) * D ** -0.5)[0].view(-1, Hkv, G, D).sum(2)
        s32 = (torch.einsum("bihd,bjhd->bhij", qs.float(), _expand(k[:, keys], G).float()) * D ** -0.5).masked_fill(~mask, float("-inf"))
        p32 = torch.exp(s32 - lse32[..., None])
        dp32 = torch.einsum("bihd,bjhd->bhij", ds.float(), _expand(v[:, keys], G).float())
        dS32 = (p32 * (dp32 - (ds.float() * o32).sum(-1).transpose(1, 2)[..., None])).to(torch.bfloat16).float()
        acc["dv_r"] += torch.einsum("bhij,bihd->bjhd", p32.to(torch.bfloat16).float(), ds.float())[0].view(-1, Hkv, G, D).sum(2).double()
        acc["dk_r"] += (torch.einsum("bhij,bihd->bjhd", dS32, qs.float()) * D ** -0.5)[0].view(-1, Hkv, G, D).sum(2).double()
    for name, got in (("dk", dk[0, keys]), ("dv", dv[0, keys])):
        truth = acc[name]
        ref = acc[name + "_r"].float().to(torch.bfloat16).double()
        e, r = rms(got.double() - truth), rms(ref - truth)
        PARITY_LOG[f"lambda full size S{S} {name} (sampled keys)"] = {"rms_err": e, "rms_err_reference_arithmetic": r,
                                                                     "ratio": e / r, "bar": 1.25}
        assert e <= 1.25 * r, f"full size {name}: rms err {e:.3e} > 1.25 x reference arithmetic's {r:.3e}"


# ---------------------------------------------------------------------------------------------------------------------
# 8. train -> save -> load -> eval
# ---------------------------------------------------------------------------------------------------------------------
def test_train_save_load_eval_round_trip(tmp_path):
    from duo_attn.patch import enable_duo_attention_eval, enable_duo_attention_training, get_full_attention_heads
    from duo_attn.patch import set_full_attention_heads
    from duo_attn.train import train_step
    from duo_attn.utils import (full_attention_heads_to_list, load_attn_pattern, save_full_attention_heads,
                                sparsify_attention_heads)

    base = make_llama(4)
    m = copy.deepcopy(base).to(device="cuda", dtype=torch.bfloat16)
    enable_duo_attention_training(m, 64, 128, 512, streaming_attn_implementation="sdpa")
    set_full_attention_heads(m, _gates_for(4))
    decoder = m.model
    _freeze_all_but_gates(decoder)
    opt = torch.optim.AdamW([p for p in decoder.parameters() if p.requires_grad], lr=0.02)
    ids = torch.randint(0, 500, (1, 512), generator=torch.Generator().manual_seed(4)).cuda()
    before = [h.detach().clone() for h in get_full_attention_heads(m)]
    loss, _, _ = train_step(decoder, ids, ids.clone(), reg_weight=0.05)
    opt.step()
    opt.zero_grad()
    assert torch.isfinite(loss)
    heads = full_attention_heads_to_list(get_full_attention_heads(m))
    assert any(abs(a - float(b)) > 0 for row, brow in zip(heads, before) for a, b in zip(row, brow.float().cpu()))
    save_full_attention_heads(heads, str(tmp_path / "full_attention_heads.tsv"))
    with open(tmp_path / "config.json", "w") as f:
        json.dump({"sink_size": 64, "recent_size": 128}, f)

    pattern, sink, recent = load_attn_pattern(str(tmp_path))
    assert pattern.shape == (4, 4) and (sink, recent) == (64, 128)
    pattern, sparsity = sparsify_attention_heads(pattern, sparsity=0.5)
    fresh = copy.deepcopy(base).to(device="cuda", dtype=torch.bfloat16)
    enable_duo_attention_eval(fresh, pattern, sink, recent)
    with torch.no_grad():
        o = fresh(input_ids=ids[:, :400], use_cache=True)
        o2 = fresh(input_ids=ids[:, 400:401], past_key_values=o.past_key_values, use_cache=True)
    assert torch.isfinite(o.logits).all() and torch.isfinite(o2.logits).all()
