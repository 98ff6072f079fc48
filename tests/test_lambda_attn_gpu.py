"""The Λ-mask (streaming) attention of retrieval-head training on the MI355X: duo_lambda_attn_{fwd,bwd}_bf16 against
dense restatements of the mask (tests/training_ref.py).

1. mask probe, exact (q = 0: P is uniform over the visible keys) — catches any added or missing key or row;
2. forward numerics against the exact-P fp32 result (helpers.attn_close with the bf16-P reference arithmetic) and the
   LSE against fp64 (bar: 2 x the torch fp32 reference's own max error);
3. backward numerics: rms(HIP - fp64 truth) <= 1.25 x rms(FA2 fp32 reference arithmetic - fp64 truth), per tensor;
5. determinism of the backward (bitwise).
Every measured ratio goes to helpers.PARITY_LOG.
"""
import math

import pytest
import torch

from helpers import PARITY_LOG, attn_close, with_rounded
from training_ref import attention_budget, dense_attention, dense_grads, fa2_reference, lambda_mask, rms

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 129, 384, 1000, 4099]
WINDOWS = [(64, 128), (128, 256), (0, 64), (100, 37), (1, 1)]
MODES = [0, 1]


def _params(sink, recent, mode):
    """the op's arguments for a (sink, recent) given in tokens: block mode takes the 128-row block counts"""
    if mode:
        return (sink + 127) // 128, (recent + 127) // 128
    return sink, recent


def _hip():
    from duo_attn import _hip

    return _hip


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sink,recent", WINDOWS)
@pytest.mark.parametrize("B", [1, 2])
def test_mask_probe_exact(B, sink, recent, mode):
    h = _hip()
    Hq, Hkv, D = 8, 2, 128
    dev = "cuda"
    ps, pr = _params(sink, recent, mode)
    for S in SIZES:
        mask = lambda_mask(S, ps, pr, mode, dev)
        n = mask.sum(1).double()                                        # visible keys per row
        q = torch.zeros(B, S, Hq, D, dtype=torch.bfloat16, device=dev)
        k = torch.randn(B, S, Hkv, D, device=dev).to(torch.bfloat16)
        j = torch.arange(S, device=dev)
        for probe, cls in (("j mod 128", j % 128), ("(j // 128) mod 128", (j // 128) % 128)):
            onehot = torch.nn.functional.one_hot(cls, 128).to(torch.bfloat16)           # [S, 128]
            v = onehot[None, :, None, :].expand(B, S, Hkv, D).contiguous()
            out, lse = h.lambda_attn_fwd(q, k, v, ps, pr, mode, D ** -0.5)
            torch.cuda.synchronize()
            counts = mask.double() @ onehot.double()                     # [S, 128]: visible keys of row i in class c
            got = torch.round(out.double() * n[None, :, None, None])
            assert torch.equal(got, counts[None, :, None, :].expand_as(got)), (
                f"S {S} {probe}: rows with a wrong key set: "
                f"{(got != counts[None, :, None, :]).any(-1).any(-1).any(0).nonzero().flatten()[:10].tolist()}")
            assert float((lse.double() - n.log()[None, None, :]).abs().max()) < 1e-5, f"S {S}: lse is not ln(n)"
        # dV[j] = sum_{i sees j} e_{i mod 128} / n_i
        v = torch.randn(B, S, Hkv, D, device=dev).to(torch.bfloat16)
        out, lse = h.lambda_attn_fwd(q, k, v, ps, pr, mode, D ** -0.5)
        dout = torch.nn.functional.one_hot(j % 128, 128).to(torch.bfloat16)[None, :, None, :].expand(B, S, Hq, D).contiguous()
        _, _, dv = h.lambda_attn_bwd(q, k, v, out, lse, dout, ps, pr, mode, D ** -0.5)
        torch.cuda.synchronize()
        w = mask.double().T / n[None, :]                                  # [j, i]
        want = w @ torch.nn.functional.one_hot(j % 128, 128).double()     # per q head; the group of 4 sums
        want = (want * (Hq // Hkv))[None, :, None, :]
        # within bf16 rounding: P = 1 / n_i rounded to bf16 (relative error <= 2^-8, the unit roundoff of an 8-bit
        # significand; every term is positive, so the sum keeps that bound) and the output rounded once more (2^-8).
        # One row added or missing moves an element by G / n_i out of a sum of a few such terms: far more than 2^-7.
        err = (dv.double() - want).abs()
        tol = 2.0 ** -7 * want.abs() + 1e-6
        assert bool((err <= tol).all()), f"S {S}: dV probe off by {float((err - tol).max()):.3e}"


def _qkv(B, S, Hq, Hkv, seed, qscale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = (torch.randn(B, S, Hq, 128, device="cuda", generator=g) * qscale).to(torch.bfloat16)
    k = torch.randn(B, S, Hkv, 128, device="cuda", generator=g).to(torch.bfloat16)
    v = torch.randn(B, S, Hkv, 128, device="cuda", generator=g).to(torch.bfloat16)
    return q, k, v


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sink,recent", WINDOWS)
@pytest.mark.parametrize("heads", [(32, 8), (8, 8), (4, 1)])
def test_forward_numerics(heads, sink, recent, mode):
    h = _hip()
    Hq, Hkv = heads
    ps, pr = _params(sink, recent, mode)
    for S in SIZES:
        mask = lambda_mask(S, ps, pr, mode, "cuda")
        # the LSE bar compares two MAXIMA of rounding noise: over a handful of rows (S = 1 has Hq of them) the max of either
        # is one draw and their ratio is noise.  Every size runs with enough batch rows for >= 4096 LSE values.
        B = max(1, math.ceil(4096 / (S * Hq)))
        for qscale in (1.0, 8.0):
            q, k, v = _qkv(B, S, Hq, Hkv, seed=S + int(qscale), qscale=qscale)
            out, lse = h.lambda_attn_fwd(q, k, v, ps, pr, mode, 128 ** -0.5)
            ref, _ = dense_attention(q, k, v, mask, dtype=torch.float32)
            ref_r, _ = dense_attention(q, k, v, mask, dtype=torch.float32, round_p=True)
            what = f"lambda fwd H{Hq}/{Hkv} S{S} sink{ps} recent{pr} mode{mode} q*{qscale:g}"
            attn_close(out.float(), ref, what, budget=with_rounded(attention_budget(q, k, v, mask), ref_r.to(torch.bfloat16).float()))
            _, lse64 = dense_attention(q, k, v, mask, dtype=torch.float64)
            _, lse32 = dense_attention(q, k, v, mask, dtype=torch.float32)
            e_hip = float((lse.double() - lse64).abs().max())
            e_ref = float((lse32.double() - lse64).abs().max())
            PARITY_LOG[what + " lse"] = {"max_err": e_hip, "max_err_fp32_reference": e_ref,
                                         "ratio": e_hip / e_ref if e_ref > 0 else 0.0, "bar": 2.0}
            assert e_hip <= 2 * e_ref, f"{what}: lse max err {e_hip:.3e} > 2 x fp32 reference's {e_ref:.3e}"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sink,recent", WINDOWS)
@pytest.mark.parametrize("heads", [(32, 8), (8, 8), (4, 1)])
def test_backward_numerics(heads, sink, recent, mode):
    h = _hip()
    Hq, Hkv = heads
    ps, pr = _params(sink, recent, mode)
    for S in SIZES[1:]:
        mask = lambda_mask(S, ps, pr, mode, "cuda")
        q, k, v = _qkv(1, S, Hq, Hkv, seed=1000 + S)
        dout = torch.randn(1, S, Hq, 128, device="cuda").to(torch.bfloat16)
        out, lse = h.lambda_attn_fwd(q, k, v, ps, pr, mode, 128 ** -0.5)
        got = h.lambda_attn_bwd(q, k, v, out, lse, dout, ps, pr, mode, 128 ** -0.5)
        truth = dense_grads(q, k, v, dout, mask, dtype=torch.float64)
        ref = fa2_reference(q, k, v, dout, mask)
        for name, g, t, r in zip(("dq", "dk", "dv"), got, truth, ref):
            e_hip, e_ref = rms(g.double() - t), rms(r.double() - t)
            what = f"lambda bwd {name} H{Hq}/{Hkv} S{S} sink{ps} recent{pr} mode{mode}"
            PARITY_LOG[what] = {"rms_err": e_hip, "rms_err_reference_arithmetic": e_ref,
                                "ratio": e_hip / e_ref if e_ref > 0 else 0.0, "bar": 1.25, "rms_truth": rms(t)}
            assert e_hip <= 1.25 * e_ref, f"{what}: rms err {e_hip:.3e} > 1.25 x reference arithmetic's {e_ref:.3e}"


@pytest.mark.parametrize("mode", MODES)
def test_backward_is_deterministic_and_takes_strided_dout(mode):
    h = _hip()
    S, Hq, Hkv = 3000, 32, 8
    ps, pr = _params(64, 128, mode)
    q, k, v = _qkv(2, S, Hq, Hkv, seed=7)
    out, lse = h.lambda_attn_fwd(q, k, v, ps, pr, mode, 128 ** -0.5)
    big = torch.randn(2, S, Hq + 8, 128, device="cuda").to(torch.bfloat16)
    dout = big[:, :, 4:4 + Hq]                                   # a view: head stride 128, token stride (Hq + 8) * 128
    a = h.lambda_attn_bwd(q, k, v, out, lse, dout, ps, pr, mode, 128 ** -0.5)
    b = h.lambda_attn_bwd(q, k, v, out, lse, dout, ps, pr, mode, 128 ** -0.5)
    c = h.lambda_attn_bwd(q, k, v, out, lse, dout.contiguous(), ps, pr, mode, 128 ** -0.5)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    out2, lse2 = h.lambda_attn_fwd(q, k, v, ps, pr, mode, 128 ** -0.5)
    assert torch.equal(out, out2) and torch.equal(lse, lse2)


def test_autograd_function_matches_the_op():
    from duo_attn.patch.streaming_attn import (generate_streaming_info_blocksparse_flash_attn, generate_streaming_mask,
                                               streaming_attn_blocksparse_flash_attn, streaming_attn_sdpa)

    h = _hip()
    S, Hq, Hkv = 700, 8, 2
    q, k, v = _qkv(1, S, Hq, Hkv, seed=3)
    dout = torch.randn(1, S, Hq, 128, device="cuda").to(torch.bfloat16)
    for fn, info, params in ((streaming_attn_sdpa, generate_streaming_mask(1024, 64, 128, "cuda"), (64, 128, 0)),
                             (streaming_attn_blocksparse_flash_attn,
                              generate_streaming_info_blocksparse_flash_attn(1, 2, Hq, "cuda"), (1, 2, 1))):
        qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
        out = fn(qa, ka, va, info)
        out.backward(dout)
        o, lse = h.lambda_attn_fwd(q, k, v, *params, 128 ** -0.5)
        want = h.lambda_attn_bwd(q, k, v, o, lse, dout, *params, 128 ** -0.5)
        assert torch.equal(out.detach(), o)
        for g, w in zip((qa.grad, ka.grad, va.grad), want):
            assert torch.equal(g, w)
