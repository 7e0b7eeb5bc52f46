"""Weight export: logical TM-layout tensors -> named, TP-sharded Param slots of the native engine.

Host-side mirror of the reference's loader for the hot path:
  * u4 packing `pack_u4_row` / AWQ unpack `_unpack_awq_gemm`  (lmdeploy/turbomind/weight_format.py:47-74)
  * QKV fusion [Q|K|V] per rank                                (lmdeploy/turbomind/builders/attention.py:65-112)
  * w1w3 gate/up column interleave for the fused-SiLU epilogue (lmdeploy/turbomind/builders/ffn.py:31-34,164-165)
  * TP sharding: column-parallel split of the output dim, row-parallel split of the input dim
    (lmdeploy/turbomind/builders/_base.py:102-113); KV heads are replicated when kv_heads < tp
    (builders/attention.py:30-50)
  * RoPE row permutation of HF q/k channels                     (lmdeploy/turbomind/models/utils.py:306-324)
  * slot hand-off with exact byte-size check                    (builders/_base.py:72-99)
"""
from __future__ import annotations

import numpy as np

AWQ_ORDER = (0, 4, 1, 5, 2, 6, 3, 7)


def unpack_awq_gemm(qw: np.ndarray) -> np.ndarray:
    """AWQ checkpoint int32[..., N/8] -> uint8[..., N]: logical column 8c+p is nibble AWQ_ORDER[p] of word c."""
    w = np.asarray(qw).view(np.uint32).astype(np.uint64)
    nib = [((w >> np.uint64(4 * i)) & np.uint64(15)).astype(np.uint8) for i in range(8)]
    return np.stack([nib[i] for i in AWQ_ORDER], axis=-1).reshape(*w.shape[:-1], -1)


def unpack_u4_cols(w: np.ndarray) -> np.ndarray:
    """int32[..., C] -> uint8[..., 8C]: element 8c+j of the last dim is nibble j of word c (sequential order: GPTQ qzeros,
    compressed-tensors weight_packed; the inverse of pack_u4_row)."""
    w = np.asarray(w).view(np.uint32).astype(np.uint64)
    nib = [((w >> np.uint64(4 * j)) & np.uint64(15)).astype(np.uint8) for j in range(8)]
    return np.stack(nib, axis=-1).reshape(*w.shape[:-1], -1)


def unpack_u4_rows(w: np.ndarray) -> np.ndarray:
    """int32[R, N] -> uint8[8R, N]: row 8r+i is nibble i of word row r (GPTQ qweight, compressed-tensors weight_zero_point)."""
    w = np.asarray(w).view(np.uint32).astype(np.uint64)
    nib = [((w >> np.uint64(4 * i)) & np.uint64(15)).astype(np.uint8) for i in range(8)]
    return np.stack(nib, axis=1).reshape(-1, w.shape[-1])


def pack_u4_row(q: np.ndarray) -> np.ndarray:
    """uint8[..., N] -> int32[..., N/8] with nibble j of word c = element 8c+j (the engine's boundary layout)."""
    g = np.asarray(q, np.uint8).reshape(*q.shape[:-1], -1, 8).astype(np.uint64)
    w = np.zeros(g.shape[:-1], np.uint64)
    for j in range(8):
        w |= g[..., j] << np.uint64(4 * j)
    return w.astype(np.uint32).view(np.int32)


def permute_qk_for_interleaved_rope(w: np.ndarray, heads: int, head_dim: int) -> np.ndarray:
    """HF rotate-half channels (j, j+D/2) -> adjacent pairs (2j, 2j+1) along the last (output) dim."""
    lead = w.shape[:-1]
    return w.reshape(*lead, heads, 2, head_dim // 2).swapaxes(-1, -2).reshape(*lead, heads * head_dim)


def interleave_gate_up(w1: np.ndarray, w3: np.ndarray) -> np.ndarray:
    out = np.empty((*w1.shape[:-1], 2 * w1.shape[-1]), w1.dtype)
    out[..., 0::2] = w1
    out[..., 1::2] = w3
    return out


def roundup128(n: int) -> int:
    return -(-int(n) // 128) * 128


def pad_f16(a: np.ndarray, shape: tuple) -> np.ndarray:
    """a in the leading corner of a +0 array of `shape` (same dtype)"""
    a = np.asarray(a)
    assert a.ndim == len(shape) and all(n <= m for n, m in zip(a.shape, shape)), f'cannot pad {a.shape} to {shape}'
    if a.shape == tuple(shape):
        return a
    out = np.zeros(shape, a.dtype)
    out[tuple(slice(0, n) for n in a.shape)] = a
    return out


def pad_mxfp4(lin: dict, N: int, K: int) -> dict:
    """MXFP4 linear {'blocks' uint8 [n, k / 2], 'scales' uint8 [n, k / 32]} -> [N, K / 2], [N, K / 32]: the pad codes are 0x00 (two e2m1
    +0) and the pad scale bytes 127 (2^0), along K and along N alike -- every pad weight dequantises to +0."""
    blocks, scales = np.asarray(lin['blocks']), np.asarray(lin['scales'])
    n, k2 = blocks.shape
    assert blocks.dtype == np.uint8 and scales.dtype == np.uint8 and scales.shape == (n, k2 // 16) and K % 32 == 0
    sc = np.full((N, K // 32), 127, np.uint8)
    sc[:n, :k2 // 16] = scales
    return dict(blocks=pad_f16(blocks, (N, K // 2)), scales=sc)


def _pad_linear(lin: dict, K: int, N: int, what: str) -> dict:
    """an fp16 linear {'w' [k, n]} or an MXFP4 one (output-major) to K x N"""
    if 'blocks' in lin:
        return pad_mxfp4(lin, N, K)
    if 'w' not in lin:
        raise NotImplementedError(f'{what}: only fp16 and MXFP4 linears are served zero-padded (AWQ / FP8 groups would straddle the pad)')
    return dict(w=pad_f16(lin['w'], (K, N)))


def pad_model_weights(weights: dict, H: int, inter: int) -> dict:
    """The weights of export_weights with every hidden axis padded from H to roundup128(H) and every FFN-width axis from `inter` to
    roundup128(inter), so that a model whose sizes are no multiple of 128 (gpt-oss: 2880 -> 2944) runs on the engine's GEMMs as they are.
    All pads are +0 (MXFP4: code 0x00 under scale byte 127): embedding columns, lm_head K rows, norm weights, w_qkv K rows, wo N columns
    and bias, router rows, expert w1w3 K rows and extra (gate, up) column pairs with +0 biases, w2 K rows, N columns and bias.  A padded
    (gate, up) pair gives act(0, 0) = 0 -- silu(0) * 0, and 0 * sigmoid(0) * (1 + 0) for gpt-oss -- so w2's pad rows see only zeros; the
    norms write +0 into the pad columns of the residual stream (tm_model_config.hidden_valid).  Sizes that are multiples of 128 already:
    the same arrays."""
    Hp, Ip = roundup128(H), roundup128(inter)
    if (Hp, Ip) == (H, inter):
        return weights

    def ffn(d: dict, what: str) -> dict:
        out = dict(d, w1w3=_pad_linear(d['w1w3'], Hp, 2 * Ip, what + '.w1w3'), w2=_pad_linear(d['w2'], Ip, Hp, what + '.w2'))
        if 'w1w3_bias' in d:
            out.update(w1w3_bias=pad_f16(d['w1w3_bias'], (2 * Ip,)), w2_bias=pad_f16(d['w2_bias'], (Hp,)))
        return out

    layers = []
    for li, L in enumerate(weights['layers']):
        if 'shared_gate' in L:
            raise NotImplementedError('a shared expert is not served zero-padded')
        if 'w' not in L['w_qkv'] or 'w' not in L['wo']:
            raise NotImplementedError(f'layers.{li}.attention: only fp16 attention linears are served zero-padded')
        P = dict(L, attn_norm=pad_f16(L['attn_norm'], (Hp,)), ffn_norm=pad_f16(L['ffn_norm'], (Hp,)),
                 w_qkv=_pad_linear(L['w_qkv'], Hp, L['w_qkv']['w'].shape[1], f'layers.{li}.w_qkv'),
                 wo=_pad_linear(L['wo'], L['wo']['w'].shape[0], Hp, f'layers.{li}.wo'))
        if 'wo_bias' in L:
            P['wo_bias'] = pad_f16(L['wo_bias'], (Hp,))
        if 'experts' in L:
            P['moe_gate'] = pad_f16(L['moe_gate'], (Hp, np.asarray(L['moe_gate']).shape[1]))
            P['experts'] = [ffn(E_, f'layers.{li}.experts.{x}') for x, E_ in enumerate(L['experts'])]
        else:
            P.update(ffn(L, f'layers.{li}.feed_forward'))
        layers.append(P)
    V = np.asarray(weights['tok_embeddings']).shape[0]
    return dict(weights, tok_embeddings=pad_f16(weights['tok_embeddings'], (V, Hp)), norm=pad_f16(weights['norm'], (Hp,)),
                output=pad_f16(weights['output'], (Hp, np.asarray(weights['output']).shape[1])), layers=layers)


def _cols(t: np.ndarray, lo: int, hi: int) -> np.ndarray:
    return t[..., lo:hi]


def _shard_linear(lin: dict, kind: str, tp: int, rank: int, group: int, col_slices=None) -> dict:
    """lin: {'q','s','z'} (u4 as uint8 [K,N], fp16 [K/g,N]) or {'w'} fp16 [K,N].
    kind 'col': take `col_slices` (list of (lo,hi)) of the output dim; 'row': split the input dim evenly."""
    out = {}
    if 'blocks' in lin:      # MXFP4 dense linears, output-major byte images: nothing to slice
        if tp != 1:
            raise ValueError(f'MXFP4 dense linears do not shard over tp = {tp}: W4A4 is served with tp = 1')
        return lin
    if 'cs' in lin:
        # e4m3 ('f8') or int8 ('i8') codes [K,N] + one fp32 scale per output channel [N]: column shards slice the scales with their
        # columns (whole (gate, up) pairs for w1w3: its slice bounds are even), row shards keep them whole
        ck = 'i8' if 'i8' in lin else 'f8'
        f8, cs = lin[ck], lin['cs']
        if kind == 'col':
            return {ck: np.concatenate([f8[:, lo:hi] for lo, hi in col_slices], axis=1),
                    'cs': np.concatenate([cs[lo:hi] for lo, hi in col_slices])}
        K = f8.shape[0]
        assert K % tp == 0 and (K // tp) % 128 == 0, 'fp8 / int8 row-parallel shards must keep whole 128-row k-blocks'
        return {ck: f8[rank * (K // tp):(rank + 1) * (K // tp)], 'cs': cs}
    if 'f8' in lin:
        # e4m3 codes [K,N] + fp32 scales of 128x128 blocks [K/128, ceil(N/128)]: a shard must keep whole blocks
        f8, bs = lin['f8'], lin['bs']
        if lin.get('gated'):
            # fused w1w3, (gate_j, up_j)-interleaved codes, scale row = [w1 blocks | w3 blocks]: rank r owns the inter
            # columns [r*I/tp, (r+1)*I/tp) of both halves
            (lo, hi), = col_slices
            assert kind == 'col' and lo % 256 == 0 and hi % 256 == 0, 'fp8 w1w3 shards must keep whole 128-column blocks'
            half = bs.shape[1] // 2
            b0, b1 = lo // 256, hi // 256
            return {'f8': f8[:, lo:hi], 'bs': np.concatenate([bs[:, b0:b1], bs[:, half + b0:half + b1]], axis=1), 'gated': True}
        if kind == 'col':
            assert all(lo % 128 == 0 and (hi % 128 == 0 or hi == f8.shape[1]) for lo, hi in col_slices), \
                'fp8 column shards must be aligned to the 128-column scale blocks'
            return {'f8': np.concatenate([f8[:, lo:hi] for lo, hi in col_slices], axis=1),
                    'bs': np.concatenate([bs[:, lo // 128:(hi + 127) // 128] for lo, hi in col_slices], axis=1)}
        K = f8.shape[0]
        assert K % tp == 0 and (K // tp) % 128 == 0, 'fp8 row-parallel shards must keep whole 128-row scale blocks'
        lo, hi = rank * (K // tp), (rank + 1) * (K // tp)
        return {'f8': f8[lo:hi], 'bs': bs[lo // 128:hi // 128]}
    if kind == 'col':
        for k, t in lin.items():
            out[k] = np.concatenate([_cols(t, lo, hi) for lo, hi in col_slices], axis=-1)
    else:
        K = (lin['q'] if 'q' in lin else lin['w']).shape[0]
        assert K % tp == 0 and (K // tp) % group == 0, 'row-parallel shard must keep whole quantisation groups'
        lo, hi = rank * (K // tp), (rank + 1) * (K // tp)
        for k, t in lin.items():
            out[k] = t[lo:hi] if k in ('q', 'w') else t[lo // group:hi // group]
    return out


def _emit(slots: dict, prefix: str, lin: dict):
    if 'blocks' in lin:      # MXFP4 experts and W4A4 dense linears in the checkpoint layout: e2m1 codes [N, K/2] + ue8m0 scale bytes [N, K/32]
        slots[prefix + '.blocks'] = np.ascontiguousarray(lin['blocks'], dtype=np.uint8)
        slots[prefix + '.scales'] = np.ascontiguousarray(lin['scales'], dtype=np.uint8)
    elif 'q' in lin:
        slots[prefix + '.qweight'] = np.ascontiguousarray(pack_u4_row(lin['q']))
        slots[prefix + '.scales'] = np.ascontiguousarray(lin['s'], dtype=np.float16)
        slots[prefix + '.zeros'] = np.ascontiguousarray(lin['z'], dtype=np.float16)
    elif 'f8' in lin:        # e4m3 codes [K,N] + fp32 128x128 block scales (lmdeploy/turbomind/weight_format.py:349-393) or [N] channel scales
        slots[prefix + '.weight'] = np.ascontiguousarray(lin['f8'], dtype=np.uint8)
        slots[prefix + '.scales'] = np.ascontiguousarray(lin['cs'] if 'cs' in lin else lin['bs'], dtype=np.float32)
    elif 'i8' in lin:        # int8 codes [K,N] + [N] channel scales (W8A8)
        slots[prefix + '.weight'] = np.ascontiguousarray(lin['i8'], dtype=np.int8)
        slots[prefix + '.scales'] = np.ascontiguousarray(lin['cs'], dtype=np.float32)
    else:
        slots[prefix + '.weight'] = np.ascontiguousarray(lin['w'], dtype=np.float16)


def export_weights(cfg, weights: dict, tp: int = 1, rank: int = 0) -> dict:
    """weights (unsharded, TM layout): {'tok_embeddings' [V,H], 'norm' [H], 'output' [H,V],
    'layers': [{'attn_norm','ffn_norm', 'w_qkv','wo','w1w3','w2': linear dicts}]} with w_qkv = [Q|K|V] along N and
    w1w3 already (gate_j, up_j)-interleaved; Qwen layers add 'qkv_bias' [Hq*D + 2*Hkv*D] (q / k permuted like w_qkv) and /
    or 'q_norm', 'k_norm' [D]; layers with attention sinks add 'sinks' [Hq], layers with an o_proj bias 'wo_bias' [H] (tp = 1); MoE layers carry 'moe_gate' [H,E] and 'experts' [{'w1w3','w2'}] instead of w1w3 / w2, Qwen2-MoE layers
    all of them: w1w3 / w2 are then the shared expert (width cfg.moe_shared_inter) next to its 'shared_gate' [H].
    gpt-oss blocks: an MXFP4 expert linear is {'blocks' uint8 [N, K/2], 'scales' uint8 [N, K/32]} (output-major, the checkpoint
    layout; w1w3's N rows (gate_j, up_j)-interleaved); with cfg.moe_bias every expert carries 'w1w3_bias' [2I] and 'w2_bias' [H] and the
    layer 'moe_gate_bias' [E] (fp32).  Neither shards: tp must be 1.
    Returns {slot name: contiguous numpy array} for this rank."""
    D = cfg.head_dim
    Hq, Hkv, I, G = cfg.q_heads, cfg.kv_heads, roundup128(cfg.inter), cfg.group
    assert Hq % tp == 0 and I % tp == 0 and cfg.vocab % tp == 0
    hq_l = Hq // tp
    if Hkv >= tp:
        assert Hkv % tp == 0
        hkv_l, kv0 = Hkv // tp, rank * (Hkv // tp)
    else:                                   # replicate kv heads
        assert tp % Hkv == 0
        hkv_l, kv0 = 1, rank // (tp // Hkv)
    q0 = rank * hq_l
    nq, nkv = Hq * D, Hkv * D
    qkv_slices = [(q0 * D, (q0 + hq_l) * D), (nq + kv0 * D, nq + (kv0 + hkv_l) * D),
                  (nq + nkv + kv0 * D, nq + nkv + (kv0 + hkv_l) * D)]
    i_l = I // tp
    S = int(getattr(cfg, 'moe_shared_inter', 0) or 0)
    s_l = S // tp
    slots = {}
    for li, L in enumerate(weights['layers']):
        p = f'layers.{li}'
        _emit(slots, p + '.attention.w_qkv', _shard_linear(L['w_qkv'], 'col', tp, rank, G, qkv_slices))
        _emit(slots, p + '.attention.wo', _shard_linear(L['wo'], 'row', tp, rank, G))
        if 'experts' in L:     # mixture of experts: replicated router, every expert sharded like the dense FFN
            fp8_channel = any('cs' in E_['w1w3'] for E_ in L['experts'])
            if tp > 1 and i_l % 128 and not fp8_channel:
                # the rank's half of a *.w1w3.scales row is i_l / 128 blocks, and the fp8 gated linear needs N = 2 * i_l % 256 == 0
                raise ValueError(f'moe experts of width {I} do not shard over tp = {tp}: {I} / {tp} = {I / tp:g} is not a multiple '
                                 f'of 128')
            if S and (S % tp or s_l % 128):
                raise ValueError(f'shared expert of width {S} does not shard over tp = {tp}: {S} / {tp} = {S / tp:g} is not a multiple '
                                 f'of 128')
            slots[p + '.moe_ffn.gate.weight'] = np.ascontiguousarray(L['moe_gate'], dtype=np.float16)
            bias = bool(getattr(cfg, 'moe_bias', 0))
            mx = any('blocks' in E_[k] for E_ in L['experts'] for k in ('w1w3', 'w2'))
            if tp > 1 and (bias or mx):
                raise ValueError(f'MXFP4 experts / expert biases do not shard over tp = {tp}: the w2 bias would need a per-rank rule')
            if bias:
                slots[p + '.moe_ffn.gate.bias'] = np.ascontiguousarray(L['moe_gate_bias'], dtype=np.float32)
            if S:              # Qwen2-MoE: the shared expert sharded like the dense FFN, its gate vector replicated
                _emit(slots, p + '.feed_forward.w1w3',
                      _shard_linear(L['w1w3'], 'col', tp, rank, G, [(2 * rank * s_l, 2 * (rank + 1) * s_l)]))
                _emit(slots, p + '.feed_forward.w2', _shard_linear(L['w2'], 'row', tp, rank, G))
                slots[p + '.moe_ffn.shared_gate.weight'] = np.ascontiguousarray(L['shared_gate'], dtype=np.float16)
            for x, E_ in enumerate(L['experts']):
                q = f'{p}.moe_ffn.experts.{x}'
                if bias:
                    slots[q + '.w1w3.bias'] = np.ascontiguousarray(E_['w1w3_bias'], dtype=np.float16)
                    slots[q + '.w2.bias'] = np.ascontiguousarray(E_['w2_bias'], dtype=np.float16)
                if mx:     # output-major byte images: nothing to slice (tp == 1)
                    _emit(slots, q + '.w1w3', E_['w1w3'])
                    _emit(slots, q + '.w2', E_['w2'])
                    continue
                _emit(slots, q + '.w1w3', _shard_linear(E_['w1w3'], 'col', tp, rank, G, [(2 * rank * i_l, 2 * (rank + 1) * i_l)]))
                _emit(slots, q + '.w2', _shard_linear(E_['w2'], 'row', tp, rank, G))
        else:
            _emit(slots, p + '.feed_forward.w1w3',
                  _shard_linear(L['w1w3'], 'col', tp, rank, G, [(2 * rank * i_l, 2 * (rank + 1) * i_l)]))
            _emit(slots, p + '.feed_forward.w2', _shard_linear(L['w2'], 'row', tp, rank, G))
        if 'qkv_bias' in L:    # the same column slices as w_qkv (replicated kv heads included)
            slots[p + '.attention.w_qkv.bias'] = np.ascontiguousarray(
                np.concatenate([L['qkv_bias'][lo:hi] for lo, hi in qkv_slices]), dtype=np.float16)
        if 'wo_bias' in L:     # added behind the all-reduce on every rank alike, which the engine does not build: tp == 1
            if tp > 1:
                raise ValueError(f'an o_proj bias does not shard over tp = {tp}')
            slots[p + '.attention.wo.bias'] = np.ascontiguousarray(L['wo_bias'], dtype=np.float16)
        if 'sinks' in L:       # one logit per q head: this rank's heads (the reference: 'sinks': SplitSide.OUTPUT)
            hq_l = Hq // tp
            slots[p + '.attention.sinks'] = np.ascontiguousarray(L['sinks'][rank * hq_l:(rank + 1) * hq_l], dtype=np.float16)
        if 'q_norm' in L:      # one head: replicated
            slots[p + '.attention.q_norm.weight'] = np.ascontiguousarray(L['q_norm'], dtype=np.float16)
            slots[p + '.attention.k_norm.weight'] = np.ascontiguousarray(L['k_norm'], dtype=np.float16)
        slots[p + '.attention_norm.weight'] = np.ascontiguousarray(L['attn_norm'], dtype=np.float16)
        slots[p + '.ffn_norm.weight'] = np.ascontiguousarray(L['ffn_norm'], dtype=np.float16)
    slots['tok_embeddings.weight'] = np.ascontiguousarray(weights['tok_embeddings'], dtype=np.float16)
    slots['norm.weight'] = np.ascontiguousarray(weights['norm'], dtype=np.float16)
    v_l = cfg.vocab // tp
    slots['output.weight'] = np.ascontiguousarray(weights['output'][:, rank * v_l:(rank + 1) * v_l], dtype=np.float16)
    return slots
