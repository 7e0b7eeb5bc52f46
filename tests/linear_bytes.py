"""What Engine.stats()['weight_bytes'] must report for a toy model, from its shapes alone: per linear, the codes plus the scales as the
checkpoint carries them (the byte column of the format table in csrc/linear.hip, restated here), plus 2 * hidden * vocab for the fp16
lm_head.  tp = 1."""


def linear_bytes(fmt, K, N):
    return {
        'u4': K * N // 2 + (K // 128) * N * 4,            # codes + (scale, zero) fp16 pairs per 128 k
        'f16': K * N * 2,
        'fp8': K * N + (K // 128) * N * 4,                # 128 x 128 block scales counted expanded per column
        'fp8_channel': K * N + 4 * N,                     # one fp32 scale per output column
        'mxfp4_expert': K * N // 2 + (K // 128) * N * 4,  # one scale byte per 32 k
        'mxfp4': K * N // 2 + N * (K // 32),
    }[fmt]


def engine_weight_bytes(cfg, fmt, expert_fmt=None):
    """cfg: anything with hidden / layers / q_heads / kv_heads / head_dim / inter / vocab (and moe_experts / moe_shared_inter)"""
    H, E = cfg.hidden, getattr(cfg, 'moe_experts', 0) or 0
    shared = getattr(cfg, 'moe_shared_inter', 0) or 0
    layer = linear_bytes(fmt, H, (cfg.q_heads + 2 * cfg.kv_heads) * cfg.head_dim) + linear_bytes(fmt, cfg.q_heads * cfg.head_dim, H)
    if E:
        xf = expert_fmt or fmt
        layer += E * (linear_bytes(xf, H, 2 * cfg.inter) + linear_bytes(xf, cfg.inter, H))
        if shared:
            layer += linear_bytes(fmt, H, 2 * shared) + linear_bytes(fmt, shared, H)
    else:
        layer += linear_bytes(fmt, H, 2 * cfg.inter) + linear_bytes(fmt, cfg.inter, H)
    return cfg.layers * layer + 2 * H * cfg.vocab
