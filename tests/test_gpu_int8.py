"""INT8 W8A8 on the GPU against tests/int8_reference.py: the per-token quantiser bit for bit (codes and scale words), the int8 x int8
GEMM bit for bit on random operands for every M and every split of K (integer accumulation is exact), the gated epilogue bit for
bit where SiLU is the identity and within the project's gated bound on random operands, the refusals at the boundary, then whole
models through Engine / pipeline()."""
import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from tests import int8_reference as r
from tests.gpu_helpers import dev, host, st

pytestmark = pytest.mark.gpu
f16, f32 = np.float16, np.float32
SENT = 0x7DAD                                                   # an fp16 NaN pattern no kernel writes


def _bits(a):
    """uint16 view with -0 mapped to +0"""
    v = np.ascontiguousarray(a, f16).view(np.uint16).copy()
    v[v == 0x8000] = 0
    return v


class _Linear:
    def __init__(self, tm, wq, sw):
        self.tm, (self.K, self.N) = tm, wq.shape
        self.h = _ffi.C.c_void_p()
        _ffi.check(tm.tm_linear_create(_ffi.C.byref(self.h), self.K, self.N, 4, 128))
        _ffi.check(tm.tm_linear_prepare_int8(self.h, dev(np.asarray(wq, np.int8)).data_ptr(), dev(np.asarray(sw, f32)).data_ptr(), st()))
        torch.cuda.synchronize()

    def __call__(self, x, gated=False, splits=0):
        """y with one NaN-poisoned row behind the last one, which must come back untouched"""
        M, ldy = x.shape[0], self.N // 2 if gated else self.N
        ws = torch.full((self.tm.tm_linear_int8_workspace(self.h, M),), 0xFF, dtype=torch.uint8, device='cuda')
        y = torch.full((M + 1, ldy), SENT, dtype=torch.int16, device='cuda').view(torch.float16)
        _ffi.check(self.tm.tm_linear_forward_int8(self.h, dev(x).data_ptr(), self.K, y.data_ptr(), ldy, M, int(gated), splits,
                                                  ws.data_ptr(), st()))
        got = host(y)
        assert (got[M].view(np.uint16) == SENT).all(), 'the row behind the last one was written'
        return got[:M]

    def close(self):
        self.tm.tm_linear_destroy(self.h)


# ---- (i) the per-token quantiser ------------------------------------------------------------------------------------------
def _tie_row(K, a):
    """(k + 0.5) 2^a for k = -126 .. 126 and one element 127 * 2^a (then zeros): sx = 2^a exactly, every element is a tie, and
    rounding to nearest even would differ from the rule in 127 places"""
    row = np.zeros(K)
    n = min(K - 1, 253)
    row[:n] = (np.arange(-126, 127)[:n] + 0.5) * 2.0**a
    row[n] = 127 * 2.0**a
    assert np.array_equal(row.astype(f16).astype(np.float64), row)
    return row.astype(f16)


@pytest.mark.parametrize('K', [128, 4224, 14336])
@pytest.mark.parametrize('M', [1, 3, 65])
def test_quant_token_bit_exact(tm, cuda, M, K):
    """codes and scale words equal the reference's: random rows of very different magnitude, an all-zero row (the clamp), a row of
    +-2^-24 (absmax below the clamp: codes +-76), the absmax in the first and in the last column, fp16 extremes, a row of exact
    ties; the row behind the last one stays poisoned"""
    rng = np.random.default_rng(M * 100003 + K)
    specials = {
        'zero': np.zeros(K, f16),
        'tiny': (np.where(rng.integers(0, 2, K) > 0, 1.0, -1.0) * 2.0**-24).astype(f16),
        'first': np.r_[f16(-7.5), (rng.standard_normal(K - 1) * 0.5).clip(-7, 7)].astype(f16),
        'last': np.r_[(rng.standard_normal(K - 1) * 0.5).clip(-7, 7), f16(9.25)].astype(f16),
        'extreme': np.r_[rng.standard_normal(5), 65504.0, rng.standard_normal(K - 9) * 100, -65504.0, rng.standard_normal(2)].astype(f16),
        'tie': _tie_row(K, -3),
    }
    assert np.isfinite(specials['extreme'].astype(f32)).all() and np.abs(specials['extreme'].astype(f32)).max() >= 65000
    q_tiny, _ = r.quant(specials['tiny'][None])
    assert np.array_equal(np.abs(q_tiny[0]), np.full(K, 76))
    kinds = list(specials)
    for first in range(0, len(kinds), M):
        x = (rng.standard_normal((M, K)) * rng.uniform(0.01, 30.0, (M, 1))).astype(f16)
        for i, kind in enumerate(kinds[first:first + M]):
            x[(7 * i + 2) % M] = specials[kind]
        xq = torch.full((M + 1, K), 0xA5, dtype=torch.uint8, device='cuda')
        sx = torch.full((M + 1,), float('nan'), dtype=torch.float32, device='cuda')
        xd = dev(np.concatenate([x, np.full((1, K), np.nan, f16)]))
        _ffi.check(tm.tm_quant_int8_token(xq.data_ptr(), sx.data_ptr(), xd.data_ptr(), K, M, K, st()))
        q_ref, s_ref = r.quant(x)
        got_q, got_s = host(xq).view(np.int8), host(sx)
        assert np.array_equal(got_s[:M].view(np.uint32), s_ref.view(np.uint32)), 'activation scales must be bit exact'
        bad = got_q[:M] != q_ref
        assert not bad.any(), (f'{int(bad.sum())} codes differ, first at {np.argwhere(bad)[0].tolist()}: got '
                               f'{got_q[:M][tuple(np.argwhere(bad)[0])]} want {q_ref[tuple(np.argwhere(bad)[0])]}')
        assert (host(xq)[M] == 0xA5).all() and np.isnan(got_s[M]), 'the row behind the last one was written'


# ---- (ii) the GEMM, bit for bit on random operands ----------------------------------------------------------------------------
SHAPES = [(128, 96), (640, 96), (128, 256), (640, 256)]
MS = (1, 33, 64, 65, 130)


def _splits(K):
    return [s for s in (0, 1, 2, 3) if not (s > 1 and K < 256 * s // 2)]


@pytest.mark.parametrize('K,N', SHAPES)
def test_linear_bit_exact(tm, cuda, K, N):
    """weight codes over [-128, 127], random fp16 activations, column scales of different size: K = 128 (one k-block) and 640 (five:
    the odd tail stage), N = 96 (three column groups under CG = 4) and 256, M over both tile forms and a second row block with one
    live row, splits 0 (heuristic) .. 3 -- the same bits for every one of them"""
    rng = np.random.default_rng(K * 3 + N)
    wq, sw = r.random_weight(rng, K, N)
    lin = _Linear(tm, wq, sw)
    try:
        for M in MS:
            x = r.random_x(rng, M, K)
            want = r.linear(x, wq, sw)
            assert np.isfinite(want.astype(f32)).all() and np.abs(want.astype(f32)).max() > 1e-2
            for splits in _splits(K):
                got = lin(x, False, splits)
                bad = _bits(got) != _bits(want)
                assert not bad.any(), (f'M {M} splits {splits}: {int(bad.sum())} outputs differ, first at {np.argwhere(bad)[0].tolist()}: '
                                       f'got {got[tuple(np.argwhere(bad)[0])]!r} want {want[tuple(np.argwhere(bad)[0])]!r}')
    finally:
        lin.close()


@pytest.mark.parametrize('K,N', [(128, 256), (640, 256), (640, 96)])
def test_linear_gated(tm, cuda, K, N):
    """the gated-SiLU epilogue: bit for bit on operands whose scaled gate accumulator is >= 32 (SiLU is the identity in fp32, the
    epilogue one fp32 product), and within the project's gated bound 2e-3 + 2^-8 |ref| on random operands (expf differs)"""
    rng = np.random.default_rng(K * 5 + N)
    wq, sw, pivot = r.exact_weight(K, N)
    lin = _Linear(tm, wq, sw)
    try:
        for M in MS:
            x = r.exact_x(M, K, pivot)
            want = r.assert_exact_gated(x, wq, sw)
            for splits in _splits(K):
                got = lin(x, True, splits)
                bad = _bits(got) != _bits(want)
                assert not bad.any(), f'exact M {M} splits {splits}: {int(bad.sum())} outputs differ, first at {np.argwhere(bad)[0].tolist()}'
    finally:
        lin.close()
    wq, sw = r.random_weight(rng, K, N)
    lin = _Linear(tm, wq, sw)
    try:
        for M in MS:
            x = r.random_x(rng, M, K)
            ref = r.linear(x, wq, sw, True).astype(f32)
            assert np.isfinite(ref).all()
            for splits in _splits(K):
                err = np.abs(lin(x, True, splits).astype(f32) - ref)
                print(f'gated random K {K} N {N} M {M} splits {splits}: max err {err.max():.3e} over |ref| up to {np.abs(ref).max():.3f}')
                assert np.all(err <= 2e-3 + 2.0**-8 * np.abs(ref)), f'M={M} splits={splits}: {err.max()}'
    finally:
        lin.close()


# ---- (iii) refusals at the boundary ------------------------------------------------------------------------------------------------
def test_boundary_refusals(tm, cuda):
    """tm_linear_forward (the weight-only entry) refuses an int8 handle by name; tm_moe_create refuses weight type 4"""
    rng = np.random.default_rng(0)
    wq, sw = r.random_weight(rng, 128, 96)
    lin = _Linear(tm, wq, sw)
    try:
        y = torch.zeros((1, 96), dtype=torch.float16, device='cuda')
        rc = tm.tm_linear_forward(lin.h, dev(np.zeros((1, 128), f16)).data_ptr(), 128, y.data_ptr(), 96, 1, 0, 0, 0, 0, None, st())
        assert rc != 0 and 'int8' in tm.tm_last_error().decode() and 'tm_linear_forward_int8' in tm.tm_last_error().decode()
    finally:
        lin.close()
    h = _ffi.C.c_void_p()
    rc = tm.tm_moe_create(_ffi.C.byref(h), 256, 128, 4, 2, 4, 1, 1.0)
    assert rc != 0 and 'int8' in tm.tm_last_error().decode()


# ---- (iv) engine and pipeline --------------------------------------------------------------------------------------------------------
TOYS = {
    'llama-sq': dict(dialect='smooth_quant'),
    'llama-d64-ct': dict(dialect='compressed-tensors', strategy='tensor', head_dim=64, q_heads=4, kv_heads=2, static=True),
    'qwen2-ct': dict(dialect='compressed-tensors', strategy='channel', arch='Qwen2ForCausalLM'),
}
PROMPT_LENS = (70, 9, 33)
STEPS = 3
_CKPT, _REF = {}, {}


def _toy(tmp_path_factory, name):
    """(path, what was written): one checkpoint per toy and session"""
    if name not in _CKPT:
        path = str(tmp_path_factory.mktemp('int8_' + name))
        _CKPT[name] = (path, r.write_checkpoint(path, seed=11, **TOYS[name]))
    return _CKPT[name]


def _reference(name, ck, kv_bits, prompts, toks):
    """logits and residual stream of the reference model, teacher-forced with the engine's tokens; computed once per token path"""
    key = (name, kv_bits, toks.tobytes())
    if key not in _REF:
        oc = r.oracle_config(ck, kv_bits)
        om = r.Int8Model(oc, r.tm_weights(ck, oc), batch=len(prompts), max_ctx=128)
        _, lg = om.forward(prompts)
        logits, resid = [lg], [None]
        for s in range(STEPS):
            _, lg = om.forward([[int(t)] for t in toks[:, s]])
            logits.append(lg)
            resid.append(om.last_resid.copy())
        _REF[key] = (logits, resid)
    return _REF[key]


@pytest.mark.parametrize('use_graph', [0, 1], ids=['eager', 'graph'])
@pytest.mark.parametrize('quant_policy', [0, 8])
@pytest.mark.parametrize('name', list(TOYS))
def test_engine_matches_reference(cuda, tmp_path_factory, name, quant_policy, use_graph):
    """toy checkpoints (smooth_quant Llama; compressed-tensors per-tensor with head_dim 64 and static scales to read past; Qwen2 with
    its QKV bias) -> read_config / load_hf_weights / export_weights -> Engine: ragged prompts in two forwards of <= 96 tokens, then 3
    decode steps, against Int8Model.  Bounds: the project's own for quantised-activation formats (tests/test_gpu_fp8_channel.py),
    3e-2 on the logits and 2e-2 on the residual stream of the decode steps"""
    from lmdeploy_amd.turbomind import checkpoint
    from lmdeploy_amd.turbomind.engine import Engine
    from lmdeploy_amd.turbomind.loader import export_weights
    path, ck = _toy(tmp_path_factory, name)
    cfg = checkpoint.read_config(path)
    assert cfg.weight_format == 'int8' and cfg.head_dim == TOYS[name].get('head_dim', 128)
    rng = np.random.default_rng(3)
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in PROMPT_LENS]
    eng = Engine.from_model_config(cfg, weight_type=4, max_batch_size=len(prompts), session_len=128, quant_policy=quant_policy,
                                   max_prefill_token_num=96, use_graph=use_graph)
    try:
        eng.load_weights(export_weights(cfg, checkpoint.load_hf_weights(path, cfg)))
        eng.start()
        eng.prefill(prompts, max_new_tokens=STEPS + 1)
        logits, resid = [eng.fetch_logits().copy()], [None]
        for _ in range(STEPS):
            eng.decode(1)
            logits.append(eng.fetch_logits().copy())
            resid.append(eng.fetch_residual(len(prompts)).copy())
        toks = eng.fetch()
    finally:
        eng.close()
    ref_logits, ref_resid = _reference(name, ck, 16 if quant_policy == 0 else quant_policy, prompts, toks)
    worst = [0.0, 0.0]
    for s in range(STEPS + 1):
        d = np.abs(logits[s].astype(f32) - ref_logits[s].astype(f32)).max()
        dr = np.abs(resid[s].astype(f32) - ref_resid[s].astype(f32)).max() if s else 0.0
        worst = [max(worst[0], d), max(worst[1], dr)]
        print(f'{name} qp {quant_policy} graph {use_graph} step {s}: max logit diff {d:.4g}, max residual diff {dr:.4g}')
    print(f'{name} qp {quant_policy} graph {use_graph}: maxima logits {worst[0]:.4g} (bound 3e-2), residual {worst[1]:.4g} (bound 2e-2)')
    assert worst[0] <= 3e-2, f'max logit diff {worst[0]}'
    assert worst[1] <= 2e-2, f'max residual diff {worst[1]}'


def test_checkpoint_through_pipeline(cuda, tmp_path_factory):
    """the smooth_quant toy through pipeline(path, model_format='int8'): first-step logits and greedy tokens against Int8Model (a
    token may be the runner-up where the reference's margin is within twice the logit bound)"""
    from lmdeploy_amd import GenerationConfig, TurbomindEngineConfig, pipeline
    path, ck = _toy(tmp_path_factory, 'llama-sq')
    rng = np.random.default_rng(21)
    prompts = [rng.integers(3, 512, n).astype(np.int32).tolist() for n in (19, 5, 40)]
    N = 4
    pipe = pipeline(path, backend_config=TurbomindEngineConfig(model_format='int8', quant_policy=8, max_batch_size=3, session_len=128))
    try:
        assert pipe.model_cfg.weight_format == 'int8'
        got = [x.token_ids for x in pipe(prompts, GenerationConfig(max_new_tokens=N, ignore_eos=True))]
        pipe.engine.prefill(prompts, max_new_tokens=2)
        lg0 = pipe.engine.fetch_logits().astype(f32)
        pipe.engine.release()
    finally:
        pipe.close()
    oc = r.oracle_config(ck, 8)
    om = r.Int8Model(oc, r.tm_weights(ck, oc), batch=3, max_ctx=128)
    _, ref = om.forward([np.asarray(p) for p in prompts])
    ref = ref.astype(f32)
    assert np.abs(lg0 - ref).max() <= 3e-2, np.abs(lg0 - ref).max()
    for s in range(N):
        for b in range(3):
            top = np.argsort(ref[b])[::-1][:2]
            margin = ref[b][top[0]] - ref[b][top[1]]
            assert got[b][s] == top[0] or (margin <= 6e-2 and got[b][s] == top[1]), (b, s, got[b][s], top, margin)
        if s + 1 < N:
            _, ref = om.forward([[got[b][s]] for b in range(3)])
            ref = ref.astype(f32)


def test_model_format_is_checked_against_the_checkpoint(cuda, tmp_path_factory):
    """model_format='fp8_channel' on an int8 checkpoint is refused before an engine is built"""
    from lmdeploy_amd import TurbomindEngineConfig, pipeline
    path, _ = _toy(tmp_path_factory, 'llama-sq')
    with pytest.raises(ValueError, match='int8'):
        pipeline(path, backend_config=TurbomindEngineConfig(model_format='fp8_channel', max_batch_size=2, session_len=128))


def test_synthetic_int8_engine(cuda):
    """tm_engine_init_synthetic fills int8 slots with usable values: finite logits that differ between prompts; stats() counts every
    decoder linear's codes and column scales (K N + 4 N) next to the fp16 lm_head; a MoE synthetic model is refused by name"""
    from lmdeploy_amd import GenerationConfig, TurbomindEngineConfig, pipeline
    pipe = pipeline('synthetic:tiny', backend_config=TurbomindEngineConfig(model_format='int8', quant_policy=8, max_batch_size=2, session_len=128))
    try:
        c = pipe.model_cfg
        shapes = [(c.hidden, (c.q_heads + 2 * c.kv_heads) * c.head_dim), (c.q_heads * c.head_dim, c.hidden), (c.hidden, 2 * c.inter),
                  (c.inter, c.hidden)]
        assert pipe.engine.stats()['weight_bytes'] == c.layers * sum(K * N + 4 * N for K, N in shapes) + 2 * c.hidden * c.vocab
        out = pipe([[1, 2, 3, 4, 5], [9, 8, 7]], GenerationConfig(max_new_tokens=3, ignore_eos=True, output_logits='generation'))
        lg = np.stack([x.logits for x in out]).astype(f32)
        assert np.isfinite(lg).all() and lg.std() > 1e-3 and not np.array_equal(lg[0], lg[1])
    finally:
        pipe.close()
    with pytest.raises(NotImplementedError, match='tiny_moe.*int8'):
        pipeline('synthetic:tiny_moe', backend_config=TurbomindEngineConfig(model_format='int8', max_batch_size=2, session_len=128))
