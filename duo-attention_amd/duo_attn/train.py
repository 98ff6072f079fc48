"""One optimisation step of retrieval-head training, in one process (restates reference ``duo_attn/train.py:98-158``
without FSDP, sequence parallelism or ``torch.distributed``).

``model``: the decoder (``model.model`` of a causal LM patched with ``enable_duo_attention_training``, as the reference
trains it, ``train.py:283``) or the causal LM itself; layers may be wrapped for activation checkpointing."""
import torch

from .loss import l1_loss
from .patch import get_full_attention_heads, map_full_attention_heads


def _gates(model):
    heads = get_full_attention_heads(model)
    if not heads:
        raise ValueError("no full_attention_heads found: call enable_duo_attention_training on the model first")
    return heads


def train_step(model, input_ids, labels, reg_weight):
    """Clamp the gates to [0, 1] in place, run the two-way forward on the doubled batch, and back-propagate
    distill loss + reg_weight * L1(gates).  ``input_ids`` / ``labels`` [B, S] (labels -100 = ignored).
    Returns (loss, distill_loss, reg_loss) as detached tensors."""
    with torch.no_grad():
        map_full_attention_heads(model, lambda x: x.clamp_(0, 1))

    if hasattr(model, "lm_head"):       # given the causal LM: train its decoder, as the reference does
        model = model.model
    bsz, seq_len = input_ids.shape
    ids = torch.cat([input_ids, input_ids], dim=0)
    position_ids = torch.arange(seq_len, device=ids.device).unsqueeze(0)
    hidden_states = model(input_ids=ids, position_ids=position_ids)[0]

    label_mask = labels.to(hidden_states.device) != -100
    num_labels = label_mask.sum()
    original = hidden_states[:bsz][label_mask].float()
    pruned = hidden_states[bsz:][label_mask].float()
    distill_loss = (original - pruned).pow(2).mean(dim=-1).sum() / num_labels

    heads = [h.to(original.device) for h in _gates(model)]
    reg_loss = l1_loss(torch.cat(heads).float())
    loss = distill_loss + reg_weight * reg_loss
    loss.backward()
    return loss.detach(), distill_loss.detach(), reg_loss.detach()
