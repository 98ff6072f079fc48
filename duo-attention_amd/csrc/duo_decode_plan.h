// Host-side split planning of the bf16 decode launches (defined in duo_decode.hip), shared with the multi-token step
// (duo_decode_multi.hip) so that both size their split-KV grids by the same rule.
#pragma once

// workgroups a decode launch aims for across both head classes (DUO_DECODE_TARGET_WGS, default 256: one per CU)
int duo_decode_target_wgs();
// splits per kv head of one class: budget_wgs / n_kv_heads, capped by the length's bucket (duo_decode_plan_bucket) and by
// max_splits; 0 for an absent class
void duo_decode_choose_splits(int n_kv_heads, int L, int max_splits, int budget_wgs, int &splits);
