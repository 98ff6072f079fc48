"""Losses of retrieval-head training (reference ``duo_attn/loss.py:1-4``)."""


def l1_loss(x):
    """mean absolute value of ``x`` (the gates' sparsity regulariser)"""
    return x.abs().sum() / x.numel()
