"""gpt-oss on the device: the RMSNorm variant for zero-padded rows bit for bit, the padded toy model through the engine against the
unpadded oracle model (tests.gpt_oss_reference) and a published-layout checkpoint through pipeline()."""
import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from lmdeploy_amd.turbomind.engine import Engine
from oracle import tm_oracle as o
from tests import gpt_oss_reference as G
from tests import row_ops_reference as rr
from tests.gpu_helpers import dev, host, st

pytestmark = pytest.mark.gpu
f16, f32 = np.float16, np.float32
NAN16 = 0x7e00


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


# ---- 5. the norm variant ------------------------------------------------------------------------------------------------------------
def _poison(a, Hv):
    a = np.array(a)
    a[..., Hv:] = np.nan
    return a


@pytest.mark.parametrize('H,Hv', [(256, 192), (2944, 2880), (4224, 4160)])
def test_rmsnorm_valid_bit_for_bit(tm, cuda, H, Hv):
    """Rows of H columns of which Hv are the row: 256 / 192 one wave with 8 pad vectors, 2944 / 2880 (gpt-oss) six waves, the last one
    partly pad, 4224 / 4160 two vectors per thread.  M 3; modes 0 (plain), 1 (fp16 hidden) and 2 (1 / 3 / 5 fp32 slabs: the clamped
    first four loads, and the loop behind them), with and without bias.  Every input's pad columns -- x, residual, hidden, slabs,
    bias, weight -- hold NaN.  On [0, Hv) y equals the kernel-order restatement of the oracle's norm on the Hv-wide rows bit for bit
    and the residual stream the oracle's; the pad columns of y and resid are +0; Hv == H is the old entry point, bit for bit."""
    assert rr.norm_geometry(H) == rr.norm_geometry(Hv), 'the restatement sums in the geometry of the launch'
    M, eps = 3, 1e-5
    rng = np.random.default_rng(H)
    w = (1 + 0.05 * rng.standard_normal(H)).astype(f16)
    w[::7] *= f16(-1)                            # negative weights: a pad computed as 0 * w would be -0
    x = rng.standard_normal((M, H)).astype(f16)
    y = torch.full((M + 1, H), NAN16, dtype=torch.int16, device='cuda')
    _ffi.check(tm.tm_rmsnorm_valid(y.data_ptr(), dev(_poison(x, Hv)).data_ptr(), dev(_poison(w, Hv)).data_ptr(), eps, M, H, Hv, st()))
    got = host(y).view(f16)
    assert (_bits(got[M]) == NAN16).all(), 'wrote past the last row'
    assert np.array_equal(_bits(got[:M, :Hv]), _bits(rr.rmsnorm_kernel_order(x[:, :Hv], w[:Hv], eps)))
    assert not _bits(got[:M, Hv:]).any(), 'pad columns of y must be +0'
    for splits in (0, 1, 3, 5):
        for bias in (False, True):
            r = rng.standard_normal((M, H)).astype(f16)
            b = (0.1 * rng.standard_normal(H)).astype(f16) if bias else None
            if splits:
                part = (0.3 * rng.standard_normal((splits, M, H))).astype(f32)
                hcur, part_d, h_d = rr.sum_partials(part), dev(_poison(part, Hv)), None
            else:
                hcur = rng.standard_normal((M, H)).astype(f16)
                part_d, h_d = None, dev(_poison(hcur, Hv))
            r_d = dev(np.concatenate([_poison(r, Hv), np.full((1, H), np.nan, f16)]))
            y = torch.full((M + 1, H), NAN16, dtype=torch.int16, device='cuda')
            _ffi.check(tm.tm_residual_rmsnorm_valid(y.data_ptr(), r_d.data_ptr(), h_d.data_ptr() if h_d is not None else None,
                                                    part_d.data_ptr() if part_d is not None else None, splits,
                                                    dev(_poison(b, Hv)).data_ptr() if bias else None, dev(_poison(w, Hv)).data_ptr(), eps, M,
                                                    H, Hv, st()))
            r_ref, y_ref = o.residual_rmsnorm(r[:, :Hv], hcur[:, :Hv], w[:Hv], eps, b[:Hv] if bias else None)
            got_r, got_y = host(r_d), host(y).view(f16)
            what = f'H {H} Hv {Hv} splits {splits} bias {bias}'
            assert np.isnan(got_r[M]).all() and (_bits(got_y[M]) == NAN16).all(), what + ': wrote past the last row'
            assert np.array_equal(_bits(got_r[:M, :Hv]), _bits(r_ref)), what + ': residual stream'
            assert np.array_equal(_bits(got_y[:M, :Hv]), _bits(rr.rmsnorm_kernel_order(r_ref, w[:Hv], eps))), what + ': y'
            assert not _bits(got_r[:M, Hv:]).any() and not _bits(got_y[:M, Hv:]).any(), what + ': pad columns must be +0'
    # Hv == H: the old entry points
    r, hcur = rng.standard_normal((M, H)).astype(f16), rng.standard_normal((M, H)).astype(f16)
    outs = []
    for valid in (False, True):
        r_d, y = dev(r.copy()), torch.zeros((M, H), dtype=torch.float16, device='cuda')
        args = (y.data_ptr(), r_d.data_ptr(), dev(hcur).data_ptr(), None, 0, None, dev(w).data_ptr(), eps, M, H)
        _ffi.check(tm.tm_residual_rmsnorm_valid(*args, H, st()) if valid else tm.tm_residual_rmsnorm(*args, st()))
        y0 = torch.zeros((M, H), dtype=torch.float16, device='cuda')
        a0 = (y0.data_ptr(), dev(x).data_ptr(), dev(w).data_ptr(), eps, M, H)
        _ffi.check(tm.tm_rmsnorm_valid(*a0, H, st()) if valid else tm.tm_rmsnorm(*a0, st()))
        outs.append((host(r_d), host(y), host(y0)))
    for a, b_ in zip(*outs):
        assert np.array_equal(_bits(a), _bits(b_))
    assert tm.tm_rmsnorm_valid(y0.data_ptr(), dev(x).data_ptr(), dev(w).data_ptr(), eps, M, H, Hv + 4, st()) == 1
    assert tm.tm_rmsnorm_valid(y0.data_ptr(), dev(x).data_ptr(), dev(w).data_ptr(), eps, M, H, H + 8, st()) == 1


# ---- 6. the engine against the oracle model -----------------------------------------------------------------------------------------
_LOADED = {}


def _loaded(form):
    if form not in _LOADED:
        mc, slots = G.load_through_reader(G.toy(0)[form])
        _LOADED[form] = (mc, slots, G.weights_from_slots(slots, mc))
    return _LOADED[form]


def _engine(mc, slots, kv_bits, use_graph, batch, session_len=256):
    eng = Engine.from_model_config(mc, weight_type=1, max_batch_size=batch, session_len=session_len,
                                   quant_policy=0 if kv_bits == 16 else kv_bits, max_prefill_token_num=96, use_graph=use_graph)
    eng.load_weights(slots)
    eng.start()
    return eng


def _engine_vs_oracle(form, kv_bits, use_graph, prompt_lens=(70, 5, 64), steps=3, session_len=256):
    mc, slots, w = _loaded(form)
    rng = np.random.default_rng(0)
    prompts = [rng.integers(0, mc.vocab, n).astype(np.int32) for n in prompt_lens]
    eng = _engine(mc, slots, kv_bits, use_graph, len(prompts), session_len)
    assert eng.cfg.model.hidden == 256 and eng.cfg.model.inter == 384 and eng.cfg.model.hidden_valid == 192
    eng.prefill(prompts, max_new_tokens=steps + 1)
    # (the last prefill iteration holds at least 139 - 96 = 43 rows)
    logits, resid = [eng.fetch_logits().copy()], [eng.fetch_residual(40).copy()]
    for _ in range(steps):
        eng.decode(1)
        logits.append(eng.fetch_logits().copy())
        resid.append(eng.fetch_residual(len(prompts)).copy())
    toks = eng.fetch()
    eng.close()
    om = G.GptOssOracleModel(G.oracle_config(mc, kv_bits, session_len + 1), w, batch=len(prompts), max_ctx=session_len)
    ids, lg = om.forward(prompts)
    for s in range(steps + 1):
        d = np.abs(logits[s].astype(f32) - lg.astype(f32))
        print(f'{form} kv {kv_bits} graph {use_graph} step {s}: max logit diff {d.max():.4f}, max |logit| {np.abs(lg.astype(f32)).max():.2f}')
        assert d.max() <= 3e-2, f'step {s}: max logit diff {d.max()}'
        top2 = np.sort(lg.astype(f32), -1)[:, -2:]
        safe = (top2[:, 1] - top2[:, 0]) > 6e-2
        assert np.array_equal(toks[safe, s], ids[safe]), f'step {s}: greedy tokens differ'
        assert not _bits(resid[s][:, mc.hidden:]).any(), f'step {s}: pad columns of the residual stream must be exactly +0'
        if s < steps:
            ids, lg = om.forward([[int(t)] for t in toks[:, s]])


@pytest.mark.parametrize('use_graph', [0, 1])
@pytest.mark.parametrize('kv_bits', [8, 16])
def test_engine_matches_oracle_padded(cuda, kv_bits, use_graph):
    """The toy (hidden 192 -> 256, inter 320 -> 384, [sliding 8, full], sinks, q / k / v / o biases, YaRN with a fractional range, 4
    MXFP4 experts top-2 with biases) from its published-layout checkpoint: prompts of 70 + 5 + 64 tokens under a 96-token prefill
    budget (two iterations), then 3 teacher-forced decode steps, eager and captured, int8 and fp16 KV.  Bounds of
    tests.test_gpu_moe_f16_engine: logits within 3e-2, tokens equal where the oracle's top-2 margin exceeds 6e-2; the pad columns of
    the residual stream are exactly 0 after every forward."""
    _engine_vs_oracle('published', kv_bits, use_graph)


def test_engine_matches_oracle_padded_fp16_experts(cuda):
    """the same model from its save_pretrained checkpoint: fp16 experts, padded like the MXFP4 ones"""
    _engine_vs_oracle('save_pretrained', 8, 1)


# ---- 7. pipeline ------------------------------------------------------------------------------------------------------------------------
def test_pipeline_serves_a_published_layout_checkpoint(cuda):
    """pipeline(path of the published-layout toy): the greedy tokens are those of an Engine loaded with the same slots; tp = 2 is
    refused by name"""
    from lmdeploy_amd import GenerationConfig, TurbomindEngineConfig, pipeline
    path = G.toy(0)['published']
    mc, slots, _ = _loaded('published')
    prompts = [list(range(3, 23)), [7, 500, 21, 9]]
    pipe = pipeline(path, backend_config=TurbomindEngineConfig(session_len=256, quant_policy=8))
    try:
        assert pipe.model_cfg.arch == 'gpt_oss' and pipe.model_cfg.layer_windows == [8, 0]
        got = [r.token_ids for r in pipe(prompts, GenerationConfig(max_new_tokens=6, ignore_eos=True))]
    finally:
        pipe.close()
    eng = Engine.from_model_config(mc, weight_type=1, max_batch_size=64, session_len=256, quant_policy=8, max_prefill_token_num=8192)
    eng.load_weights(slots)
    eng.start()
    eng.prefill([np.asarray(p, np.int32) for p in prompts], max_new_tokens=6)
    eng.decode(5)
    want = eng.fetch()
    eng.close()
    assert [list(t) for t in got] == want.tolist()
    with pytest.raises(NotImplementedError, match='tp = 2'):
        pipeline(path, backend_config=TurbomindEngineConfig(session_len=256, quant_policy=8, tp=2))
