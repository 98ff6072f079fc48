"""Retrieval-head training on the host (no GPU): the mask helpers against the reference's own output, the two-way
plumbing with a dense test backend (tests/training_ref.py), argument validation, and the small pieces (l1_loss,
full_attention_heads_to_list, train_step)."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from training_ref import DenseLambdaBackend, distill_loss, lambda_mask, make_llama, model_two_way_hidden

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_golden import REF  # noqa: E402

REF_STREAMING = os.path.join(REF, "duo_attn", "patch", "streaming_attn.py")


def _ref_streaming():
    """the reference's streaming_attn.py itself (it imports only torch; its optional imports fall back to None)"""
    spec = importlib.util.spec_from_file_location("_ref_streaming_attn", REF_STREAMING)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_generate_streaming_mask_matches_the_fixture():
    from duo_attn.patch.streaming_attn import generate_streaming_mask

    fx = np.load(os.path.join(HERE, "golden", "training_masks.npz"))
    assert len(fx.files) >= 5
    for key in fx.files:
        _, n, sink, recent = key.split("_")
        got = generate_streaming_mask(int(n), int(sink), int(recent), "cpu")
        assert got.dtype == torch.bool and got.numpy().shape == fx[key].shape
        assert np.array_equal(got.numpy(), fx[key]), key
        assert got.duo_lambda == (int(sink), int(recent), 0)
        # the tests' restatement of the token mode is the same mask
        N = got.shape[-1]
        assert torch.equal(lambda_mask(N, int(sink), int(recent), 0), got[0, 0])


@pytest.mark.skipif(not os.path.exists(REF_STREAMING), reason="the reference checkout is not present")
def test_mask_helpers_match_the_live_reference():
    from duo_attn.patch import streaming_attn as S

    ref = _ref_streaming()
    for n, sink, recent in [(1, 1, 1), (9, 4, 0), (33, 0, 8), (128, 64, 128), (257, 100, 37), (500, 128, 256)]:
        assert torch.equal(S.generate_streaming_mask(n, sink, recent, "cpu"), ref.generate_streaming_mask(n, sink, recent, "cpu"))
    for nsb, nlb, nh in [(1, 1, 4), (1, 2, 32), (0, 3, 8)]:
        a = S.generate_streaming_info_blocksparse_flash_attn(nsb, nlb, nh, "cpu")
        b = ref.generate_streaming_info_blocksparse_flash_attn(nsb, nlb, nh, "cpu")
        assert a.dtype == b.dtype and torch.equal(a, b)


def test_mask_parameters_are_read_once_from_a_foreign_mask():
    from duo_attn.patch import streaming_attn as S

    for n, sink, recent in [(64, 4, 16), (100, 0, 7), (40, 3, 100)]:
        m = S.generate_streaming_mask(n, sink, recent, "cpu").clone()      # (clone drops the host attribute)
        assert not hasattr(m, "duo_lambda")
        p = S._token_params(m)
        rebuilt = lambda_mask(m.shape[-1], p[0], p[1], 0)
        assert torch.equal(rebuilt, m[0, 0]) and m.duo_lambda == p
    info = S.generate_streaming_info_blocksparse_flash_attn(2, 3, 4, "cpu").clone()
    assert S._block_params(info) == (2, 3, 1)


# ---------------------------------------------------------------------------------------------------------------------
# two-way plumbing on the CPU with the dense test backend
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def dense_backend():
    from duo_attn import backend

    backend._set_backend_for_testing(DenseLambdaBackend())
    yield
    backend._set_backend_for_testing(None)


def _small_model(seed=0):
    return make_llama(seed, layers=2, hidden=256, heads=4, kv_heads=2, inter=512, vocab=100).float()


@pytest.mark.parametrize("impl,sink,recent,S", [("sdpa", 16, 32, 150), ("blocksparse", 64, 128, 300)])
def test_two_way_plumbing(dense_backend, impl, sink, recent, S):
    from duo_attn.patch import (enable_duo_attention_training, get_full_attention_heads, map_full_attention_heads,
                                set_full_attention_heads)

    model = _small_model()
    ids = torch.randint(0, 100, (1, S), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        plain = model.model(input_ids=ids).last_hidden_state
    enable_duo_attention_training(model, sink, recent, 512, initial_value=1.0, streaming_attn_implementation=impl)
    heads = get_full_attention_heads(model)
    assert len(heads) == 2 and all(isinstance(h, torch.nn.Parameter) and h.shape == (2,) for h in heads)
    assert all(torch.equal(h.detach(), torch.ones(2)) for h in heads)

    decoder = model.model                                   # train.py:283-292: freeze everything but the gates
    for p in decoder.parameters():
        p.requires_grad = False
    for n, p in decoder.named_parameters():
        if "full_attention_heads" in n:
            p.requires_grad = True
    assert {n for n, p in decoder.named_parameters() if p.requires_grad} == {
        f"layers.{i}.self_attn.full_attention_heads" for i in range(2)}

    set_full_attention_heads(model, [torch.tensor([1.7, -0.3]), torch.tensor([0.5, 2.0])])
    map_full_attention_heads(model, lambda x: x.data.clamp_(0, 1))
    assert [h.detach().tolist() for h in get_full_attention_heads(model)] == [[1.0, 0.0], [0.5, 1.0]]

    gates = [torch.tensor([0.3, 0.7]), torch.tensor([0.6, 0.25])]
    set_full_attention_heads(model, gates)
    out = decoder(input_ids=torch.cat([ids, ids]), position_ids=torch.arange(S)[None])[0]
    # the full half is the unpatched model's forward
    rel = float((out[:1].detach() - plain).norm() / plain.norm())
    assert rel < 1e-5, rel
    # gate gradients equal those of the fp64 restatement (same dense arithmetic, so only fp32 rounding separates them)
    loss = distill_loss(out, 1)
    loss.backward()
    got = torch.cat([h.grad for h in get_full_attention_heads(model)])
    mode = 1 if impl == "blocksparse" else 0
    ps, pr = ((sink + 127) // 128, (recent + 127) // 128) if mode else (sink, recent)
    g64 = [g.double().requires_grad_(True) for g in gates]
    ref_model = _small_model()
    h64 = model_two_way_hidden(ref_model, ids, g64, ps, pr, mode, torch.float64)
    distill_loss(h64, 1).backward()
    want = torch.cat([g.grad for g in g64])
    assert float(want.abs().min()) > 0
    assert float((got.double() - want).norm() / want.norm()) < 1e-4


def test_train_step_on_the_host(dense_backend):
    from duo_attn.loss import l1_loss
    from duo_attn.patch import enable_duo_attention_training, get_full_attention_heads, set_full_attention_heads
    from duo_attn.train import train_step
    from duo_attn.utils import full_attention_heads_to_list

    model = _small_model(3)
    enable_duo_attention_training(model, 16, 32, 256, initial_value=1.0, streaming_attn_implementation="sdpa")
    decoder = model.model
    for n, p in decoder.named_parameters():
        p.requires_grad = "full_attention_heads" in n
    set_full_attention_heads(model, [torch.tensor([1.5, 0.4]), torch.tensor([-1.0, 0.6])])
    ids = torch.randint(0, 100, (1, 120), generator=torch.Generator().manual_seed(2))
    labels = ids.clone()
    labels[:, :10] = -100
    loss, distill, reg = train_step(decoder, ids, labels, reg_weight=0.05)
    heads = get_full_attention_heads(model)
    assert torch.equal(torch.stack([h.detach() for h in heads]), torch.tensor([[1.0, 0.4], [0.0, 0.6]]))  # clamped first
    assert all(h.grad is not None and bool(h.grad.abs().sum() > 0) for h in heads)
    assert torch.allclose(reg, l1_loss(torch.cat([h.detach() for h in heads]).float()))
    assert torch.allclose(loss, distill + 0.05 * reg)
    listed = full_attention_heads_to_list(list(heads))
    assert listed == [[1.0, 0.4000000059604645], [0.0, 0.6000000238418579]]


def test_l1_loss_and_heads_to_list_follow_the_reference():
    from duo_attn.loss import l1_loss
    from duo_attn.utils import full_attention_heads_to_list

    x = torch.tensor([-1.0, 2.0, 0.5, -0.25])
    assert float(l1_loss(x)) == pytest.approx(3.75 / 4)
    heads = [torch.tensor([0.25, 1.0], dtype=torch.bfloat16, requires_grad=True), torch.tensor([0.5, 0.0])]
    out = full_attention_heads_to_list(heads)
    assert out is heads and out == [[0.25, 1.0], [0.5, 0.0]]


# ---------------------------------------------------------------------------------------------------------------------
# argument validation
# ---------------------------------------------------------------------------------------------------------------------
def test_the_bare_object_call_still_raises_not_implemented():
    from duo_attn.patch import enable_duo_attention_training

    with pytest.raises(NotImplementedError):
        enable_duo_attention_training(type("M", (), {"config": type("C", (), {"model_type": "llama"})})(), 1, 1, 1)


def test_unsupported_models_are_refused_before_anything_changes():
    from duo_attn.patch import enable_duo_attention_training
    from transformers import LlamaConfig, LlamaForCausalLM

    cfg = LlamaConfig(vocab_size=50, hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2,
                      num_key_value_heads=1)                       # head_dim 64
    m = LlamaForCausalLM(cfg)
    fwd = m.model.layers[0].self_attn.forward
    with pytest.raises(NotImplementedError, match="head_dim"):
        enable_duo_attention_training(m, 4, 8, 64)
    assert m.model.layers[0].self_attn.forward == fwd and not hasattr(m.model.layers[0].self_attn, "full_attention_heads")

    m = _small_model()
    m.model.layers[1].self_attn.q_proj = torch.nn.Identity()
    with pytest.raises(NotImplementedError, match="projections"):
        enable_duo_attention_training(m, 4, 8, 64)
    assert not hasattr(m.model.layers[0].self_attn, "full_attention_heads")


def test_implementation_name_window_and_ulysses_arguments():
    from duo_attn.patch import enable_duo_attention_training

    m = _small_model()
    with pytest.raises(ValueError, match="Unsupported streaming attention implementation"):
        enable_duo_attention_training(m, 4, 8, 64, streaming_attn_implementation="xformers")
    with pytest.raises(ValueError):
        enable_duo_attention_training(m, 0, 0, 64)
    assert not hasattr(m.model.layers[0].self_attn, "full_attention_heads")
    # one process (no process group): Ulysses is the identity, train.py:273-281's call shape works
    enable_duo_attention_training(m, 64, 128, 256, initial_value=0.5, enable_ulysses_attention=True)
    a = m.model.layers[0].self_attn
    assert a._duo_lambda == (1, 1, 1) and a.streaming_mask.tolist() == [1, 1] * 4
    assert torch.equal(a.full_attention_heads.detach(), torch.full((2,), 0.5))
    m = _small_model()
    enable_duo_attention_training(m, 100, 37, 300, streaming_attn_implementation="sdpa")
    a = m.model.layers[1].self_attn
    assert a._duo_lambda == (100, 37, 0) and a.streaming_mask.shape == (1, 1, 304, 304)


def test_mistral_family_dispatches_to_the_same_patch(dense_backend):
    from duo_attn.patch import enable_duo_attention_training, get_full_attention_heads
    from duo_attn.patch.mistral import enable_mistral_duo_attention_training, mistral_duo_attention_forward_two_way
    from transformers import MistralConfig, MistralForCausalLM

    assert callable(enable_mistral_duo_attention_training) and callable(mistral_duo_attention_forward_two_way)
    cfg = MistralConfig(vocab_size=50, hidden_size=256, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2,
                        num_key_value_heads=1, head_dim=128, sliding_window=None)
    m = MistralForCausalLM(cfg).float()
    enable_duo_attention_training(m, 8, 16, 64, initial_value=0.4, streaming_attn_implementation="sdpa")
    ids = torch.randint(0, 50, (1, 40))
    out = m.model(input_ids=torch.cat([ids, ids]))[0]
    out[1:].sum().backward()
    assert get_full_attention_heads(m)[0].grad is not None
