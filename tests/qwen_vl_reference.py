"""Qwen2-VL / Qwen2.5-VL language models restated on the oracle's primitives, for the M-RoPE / image-embedding tests.

The contract, in numpy on oracle.tm_oracle:
  * M-RoPE in sections: frequency pair j of a head -- (x[2j], x[2j+1]) in the engine's interleaved layout -- takes its table row from
    the t coordinate for j < s_t, from h for j < s_t + s_h, from w behind; the row is clamp(c, 0, max_pos - 1); the (cos, sin) is entry
    j of that row of the fp16 table (o.rope_cos_sin); the rotation is o.rope_apply's.  K / V land at the LINEAR position.
  * position delta: a token without explicit coordinates at linear position p sits at p + delta on all three axes.
  * embeddings: a prompt row inside an embedding range is the request's fp16 row, the token id there is not read.
Everything else is the Qwen2 decoder of tests/qwen_reference.py (bias before RoPE).

Also here: the toy transformers Qwen2VLForConditionalGeneration the CPU tests compare against, and its writer in both on-disk forms.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass

import numpy as np

from oracle import tm_oracle as o
from tests.qwen_reference import QwenConfig, QwenOracleModel, prologue

f16, f32 = np.float16, np.float32

SECTIONS = (16, 24, 24)


@dataclass
class QwenVLConfig(QwenConfig):
    mrope_section: tuple = None


def axis_of_pair(sections, pairs: int) -> np.ndarray:
    """[pairs] -> 0 (t) | 1 (h) | 2 (w)"""
    j = np.arange(pairs)
    return np.where(j < sections[0], 0, np.where(j < sections[0] + sections[1], 1, 2))


def mrope_cos_sin(rope: o.RopeParam, coords, sections, max_pos: int):
    """coords int [3, n] -> (cos, sin) fp16 [n, D / 2]: per column the row of its section's coordinate, clamped to the table"""
    coords = np.clip(np.asarray(coords, np.int64), 0, max_pos - 1)
    cs = [o.rope_cos_sin(rope, coords[a]) for a in range(3)]
    ax = axis_of_pair(sections, rope.dim // 2)[None, :]
    cos = np.where(ax == 0, cs[0][0], np.where(ax == 1, cs[1][0], cs[2][0]))
    sin = np.where(ax == 0, cs[0][1], np.where(ax == 1, cs[1][1], cs[2][1]))
    return cos, sin


def seq_coords(coords, delta: int, lo: int, hi: int) -> np.ndarray:
    """[3, hi - lo] for the linear positions [lo, hi): the given coordinates, then p + delta on all three axes"""
    coords = np.zeros((3, 0), np.int64) if coords is None else np.asarray(coords, np.int64).reshape(3, -1)
    p = np.arange(lo, hi)
    lin = np.broadcast_to(p + delta, (3, len(p)))
    given = coords[:, np.minimum(p, max(coords.shape[1] - 1, 0))] if coords.shape[1] else lin
    return np.where(p[None, :] < coords.shape[1], given, lin)


class VLSeqModel(QwenOracleModel):
    """one sequence (batch 1) of a Qwen2-VL language model: `coords` [3, n_pos] or None, `delta`, `emb` {linear position: fp16 row};
    `sections` None = plain RoPE (a model without sections), `max_pos` = rows of the engine's table"""

    def setup(self, sections, max_pos, coords=None, delta=0, emb=None):
        self.sections, self.max_pos, self.coords, self.delta, self.emb = sections, max_pos, coords, int(delta), dict(emb or {})
        return self

    def forward(self, ids_per_seq, decode_splits=1):
        cfg = self.cfg
        D, Hq, Hkv = cfg.head_dim, cfg.q_heads, cfg.kv_heads
        (t,) = ids_per_seq
        n, hist = len(t), self.seq_len[0]
        resid = o.embedding_lookup(self.w['tok_embeddings'], np.asarray(t, np.int64)).copy()
        for p, row in self.emb.items():
            if hist <= p < hist + n:
                resid[p - hist] = np.asarray(row, f16)
        x = o.rmsnorm(resid, self.w['layers'][0]['attn_norm'], cfg.rms_eps)
        if self.sections is None:
            cos, sin = o.rope_cos_sin(cfg.rope, np.minimum(np.arange(hist, hist + n), self.max_pos - 1))
        else:
            cos, sin = mrope_cos_sin(cfg.rope, seq_coords(self.coords, self.delta, hist, hist + n), self.sections, self.max_pos)
        for li, Lw in enumerate(self.w['layers']):
            qkv = o._linear(x, Lw['w_qkv'], cfg.group)
            q, k, v = prologue(qkv[:, :Hq * D].reshape(n, Hq, D), qkv[:, Hq * D:(Hq + Hkv) * D].reshape(n, Hkv, D),
                               qkv[:, (Hq + Hkv) * D:].reshape(n, Hkv, D), Lw, cfg.rms_eps)
            q = o.rope_apply(q, cos, sin)
            o.process_kv(self.cache, self.tables[0], li, k, v, cos, sin, hist)
            if n == 1:
                kv = [self.cache.load_dequant(self.tables[0], li, hd, 0, hist + 1, 'decode') for hd in range(Hkv)]
                attn = o.decode_attention(q[0], np.stack([a for a, _ in kv]), np.stack([c for _, c in kv]), self.c,
                                          decode_splits).reshape(1, -1)
            else:
                Kf, Vf = o.flatten_kv(self.cache, self.tables[0], li, hist + n)
                attn = o.prefill_attention(q, Kf, Vf, hist, self.c).reshape(n, -1)
            resid, x = o.residual_rmsnorm(resid, o._linear(attn, Lw['wo'], cfg.group), Lw['ffn_norm'], cfg.rms_eps)
            d = o._linear(o._linear(x, Lw['w1w3'], cfg.group, gated=True), Lw['w2'], cfg.group)
            nxt = self.w['layers'][li + 1]['attn_norm'] if li + 1 < cfg.layers else self.w['norm']
            resid, x = o.residual_rmsnorm(resid, d, nxt, cfg.rms_eps)
        self.last_resid = resid
        self.all_logits = o.lm_head(x, self.w['output'])
        self.seq_len[0] += n
        return o.greedy(self.all_logits[-1:]), self.all_logits[-1:]


class PerSequenceVLOracle:
    """like rope_scaling_reference.PerSequenceOracle: one VLSeqModel per sequence; `mm[b]` = dict(coords=, delta=, emb=) or None"""

    def __init__(self, cfg, weights, mm, max_ctx: int, sections=SECTIONS, max_pos: int = None):
        self.models = [VLSeqModel(cfg, weights, batch=1, max_ctx=max_ctx).setup(sections, max_pos or max_ctx + 1, **(m or {})) for m in mm]

    def forward(self, ids_per_seq):
        ids, logits = [], []
        for m, t in zip(self.models, ids_per_seq):
            i, lg = m.forward([t])
            ids.append(i[0])
            logits.append(lg[0])
        return np.asarray(ids), np.stack(logits)


def engine_mm(mm, prompt_len, hidden):
    """one oracle `mm` entry -> what Engine.set_multimodal takes: the override rows become ranges of consecutive positions"""
    m = mm or {}
    pos = sorted((m.get('emb') or {}))
    ranges, embs = [], []
    for p in pos:
        if ranges and ranges[-1][1] == p:
            ranges[-1][1] = p + 1
            embs[-1].append(m['emb'][p])
        else:
            ranges.append([p, p + 1])
            embs.append([m['emb'][p]])
    return dict(prompt_len=prompt_len, input_embeddings=[np.asarray(e, f16).reshape(-1, hidden) for e in embs],
                input_embedding_ranges=[tuple(r) for r in ranges], mrope_position_ids=m.get('coords'),
                mrope_position_delta=int(m.get('delta') or 0))


# ---- the toy transformers model -------------------------------------------------------------------------------------------------------
V, H, IMAGE, VSTART, VEND = 1024, 256, 5, 3, 4
TOY_PROMPT = [1, 2, VSTART] + [IMAGE] * 6 + [VEND, 7, 8, 9]      # one 1 x 4 x 6 grid, merge 2 -> 6 image tokens
TOY_GRID = [[1, 4, 6]]


def build_toy(seed: int, q_heads: int = 2, kv_heads: int = 1, qk_scale: float = 1.0):
    """Qwen2VLForConditionalGeneration, fp32, eager: text hidden 256, 2 layers, heads of 128, mrope_section (16, 24, 24); vision depth 1.
    qk_scale multiplies the q / k projections (weights and biases): sharper attention, so that positions matter"""
    import torch
    from transformers import Qwen2VLConfig, Qwen2VLForConditionalGeneration
    cfg = Qwen2VLConfig(
        text_config=dict(hidden_size=H, num_hidden_layers=2, num_attention_heads=q_heads, num_key_value_heads=kv_heads, intermediate_size=512,
                         vocab_size=V, max_position_embeddings=512, tie_word_embeddings=False, bos_token_id=None, eos_token_id=None,
                         rope_parameters=dict(rope_type='default', rope_theta=10000.0, mrope_section=list(SECTIONS))),
        vision_config=dict(depth=1, embed_dim=64, hidden_size=H, num_heads=2, mlp_ratio=2, patch_size=14, spatial_merge_size=2,
                           temporal_patch_size=2, in_channels=3),
        image_token_id=IMAGE, video_token_id=6, vision_start_token_id=VSTART, vision_end_token_id=VEND)
    cfg._attn_implementation = 'eager'
    torch.manual_seed(seed)
    model = Qwen2VLForConditionalGeneration(cfg).float().eval()
    with torch.no_grad():
        for name, p in model.named_parameters():
            if '.bias' in name and 'language_model' in name:      # the initialiser leaves biases 0: make the q / k / v bias count
                p.normal_(0.0, 0.1)
            if 'language_model' in name and ('q_proj' in name or 'k_proj' in name):
                p.mul_(qk_scale)
    return model


def language_state(model) -> dict:
    """{name relative to the language model's `model.`: fp16 numpy} + lm_head.weight, and the vision tensors under 'visual.'"""
    lang, vis = {}, {}
    for k, v in model.state_dict().items():
        a = v.detach().float().numpy()
        if k.startswith('model.language_model.'):
            lang[k[len('model.language_model.'):]] = a.astype(f16)
        elif k.startswith('model.visual.'):
            vis[k[len('model.visual.'):]] = a.astype(f16)
        elif k == 'lm_head.weight':
            lang['lm_head.weight'] = a.astype(f16)
    return lang, vis


def round_to_f16(model):
    """the model's parameters rounded to fp16 values (kept in fp32): both sides of a comparison then hold the same numbers"""
    import torch
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(p.half().float())
    return model


def write_checkpoint(model, path: str, form: str, awq: bool = False):
    """form 'nested': the language config under text_config (rope_parameters), weights under model.language_model. / model.visual.;
    form 'published': the language config at the top level (rope_scaling {type: mrope} + rope_theta), weights under model. / visual.
    awq: the language model's projections as AWQ g128 (the vision tower stays fp16, as published AWQ checkpoints have it)"""
    from safetensors.numpy import save_file
    os.makedirs(path, exist_ok=True)
    lang, vis = language_state(model)
    lp, vp = ('model.language_model.', 'model.visual.') if form == 'nested' else ('model.', 'visual.')
    tensors = {}
    for k, v in lang.items():
        name = k if k == 'lm_head.weight' else lp + k
        if awq and k.endswith('_proj.weight'):
            q, s, z, _ = o.quantize_groupwise_u4(np.ascontiguousarray(v.T), 128)
            pre = name[:-len('.weight')]
            tensors[pre + '.qweight'], tensors[pre + '.qzeros'], tensors[pre + '.scales'] = o.pack_awq_gemm(q), o.pack_awq_gemm(z.astype(np.uint8)), s
        else:
            tensors[name] = v
    tensors.update({vp + k: v for k, v in vis.items()})
    save_file(tensors, os.path.join(path, 'model.safetensors'))
    c = json.loads(model.config.to_json_string())
    c['architectures'] = [type(model).__name__]
    if form == 'published':
        text = c.pop('text_config')
        rp = text.pop('rope_parameters')
        for k in ('model_type', 'bos_token_id', 'eos_token_id', 'pad_token_id'):
            text.pop(k, None)
        c.update(text, rope_theta=rp['rope_theta'], rope_scaling=dict(type='mrope', mrope_section=rp['mrope_section']))
    if awq:
        c['quantization_config'] = {'quant_method': 'awq', 'bits': 4, 'group_size': 128, 'zero_point': True, 'version': 'gemm'}
    with open(os.path.join(path, 'config.json'), 'w') as f:
        json.dump(c, f)
    return path


def hf_rope_index(model, ids, grid):
    """(position ids int [3, n], delta) as transformers computes them"""
    import torch
    t = torch.tensor([list(ids)])
    pos, delta = model.model.get_rope_index(t, (t == IMAGE).int(), image_grid_thw=torch.tensor(grid))
    return pos[:, 0].numpy(), int(delta.reshape(-1)[0])


def hf_image_features(model, pixel_values, grid) -> np.ndarray:
    import torch
    with torch.no_grad():
        out = model.model.visual(torch.as_tensor(pixel_values), grid_thw=torch.tensor(grid))
    out = getattr(out, 'pooler_output', out)
    return (torch.cat(list(out)) if isinstance(out, (list, tuple)) else out).float().numpy()


def hf_logits(model, ids, emb_rows: dict, pos) -> np.ndarray:
    """fp32 logits [n, V] of the language half fed inputs_embeds (token rows, `emb_rows` {position: row} substituted) + 3-D positions"""
    import torch
    with torch.no_grad():
        e = model.model.language_model.embed_tokens(torch.tensor([list(ids)])).clone()
        for p, row in emb_rows.items():
            e[0, p] = torch.as_tensor(np.asarray(row, f32))
        return model(inputs_embeds=e, position_ids=torch.tensor(np.array(pos, np.int64)).reshape(3, 1, -1), use_cache=False).logits[0].float().numpy()


def weights_from_slots(slots: dict, mc) -> dict:
    """the engine's fp16 slots of a Qwen2(-VL) language model -> the oracle's weights"""
    layers = []
    for li in range(mc.layers):
        p = f'layers.{li}'
        layers.append(dict(attn_norm=slots[p + '.attention_norm.weight'], ffn_norm=slots[p + '.ffn_norm.weight'],
                           w_qkv=dict(w=slots[p + '.attention.w_qkv.weight']), qkv_bias=slots[p + '.attention.w_qkv.bias'],
                           wo=dict(w=slots[p + '.attention.wo.weight']), w1w3=dict(w=slots[p + '.feed_forward.w1w3.weight']),
                           w2=dict(w=slots[p + '.feed_forward.w2.weight'])))
    return dict(tok_embeddings=slots['tok_embeddings.weight'], layers=layers, norm=slots['norm.weight'], output=slots['output.weight'])


def oracle_config(mc, kv_bits: int = 16) -> QwenVLConfig:
    return QwenVLConfig(hidden=mc.hidden, layers=mc.layers, q_heads=mc.q_heads, kv_heads=mc.kv_heads, head_dim=mc.head_dim, inter=mc.inter,
                        vocab=mc.vocab, rms_eps=mc.rms_eps, rope=o.RopeParam(mc.head_dim, mc.rope.base), kv_bits=kv_bits,
                        weight_format='f16', attn_bias=1, mrope_section=tuple(mc.mrope_section))


def load_through_reader(path: str):
    """read_config + load_hf_weights + export_weights -> (checkpoint.ModelConfig, slots)"""
    from lmdeploy_amd.turbomind import checkpoint
    from lmdeploy_amd.turbomind.loader import export_weights
    mc = checkpoint.read_config(path)
    return mc, export_weights(mc, checkpoint.load_hf_weights(path, mc))


_TOYS = {}


def toy(seed: int = 0, **kw):
    """the toy of `seed` (parameters rounded to fp16 values), built and written once per process -> dict(model, nested=dir, published=dir)"""
    key = (seed, tuple(sorted(kw.items())))
    if key not in _TOYS:
        import atexit
        import shutil
        import tempfile
        root = tempfile.mkdtemp(prefix='qwen_vl_toy_')
        atexit.register(shutil.rmtree, root, ignore_errors=True)
        model = round_to_f16(build_toy(seed, **kw))
        _TOYS[key] = dict(model=model, root=root, nested=write_checkpoint(model, os.path.join(root, 'nested'), 'nested'),
                          published=write_checkpoint(model, os.path.join(root, 'published'), 'published'))
    return _TOYS[key]
