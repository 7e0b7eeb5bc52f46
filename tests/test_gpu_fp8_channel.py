"""Channel-scaled FP8 (per-tensor and per-channel FP8 checkpoints) on the GPU against tests/fp8_channel_reference.py:
the per-token quantiser bit for bit, the channel-scaled fp8 x fp8 GEMM (plain and grouped) bit for bit on exactly summable
operands and within the block-scaled test's bounds on random ones, then whole models through Engine / pipeline()."""
import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from oracle import tm_oracle as o
from tests import fp8_channel_reference as r
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
        _ffi.check(tm.tm_linear_create(_ffi.C.byref(self.h), self.K, self.N, 2, 128))
        _ffi.check(tm.tm_linear_prepare_fp8_channel(self.h, dev(wq).data_ptr(), dev(np.asarray(sw, f32)).data_ptr(), st()))
        torch.cuda.synchronize()

    def __call__(self, x, gated=False, splits=0):
        """y with one NaN-poisoned row behind the last one, which must come back untouched"""
        M, ldy = x.shape[0], self.N // 2 if gated else self.N
        ws = torch.full((self.tm.tm_linear_fp8_workspace(self.h, M),), 0xFF, dtype=torch.uint8, device='cuda')
        y = torch.full((M + 1, ldy), SENT, dtype=torch.int16, device='cuda').view(torch.float16)
        _ffi.check(self.tm.tm_linear_forward_fp8(self.h, dev(x).data_ptr(), self.K, y.data_ptr(), ldy, M, int(gated), splits,
                                                 ws.data_ptr(), st()))
        got = host(y)
        assert (got[M].view(np.uint16) == SENT).all(), 'the row behind the last one was written'
        return got[:M]

    def close(self):
        self.tm.tm_linear_destroy(self.h)


# ---- (i) the per-token quantiser ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [128, 4224, 14336])
@pytest.mark.parametrize('M', [1, 3, 65])
def test_quant_token_bit_exact(tm, cuda, M, K):
    """codes and scale words equal the reference's: random rows of very different magnitude, an all-zero row (the clamp), the
    absmax in the first and in the last column, fp16 extremes, fp16 subnormals; the row behind the last one stays poisoned"""
    rng = np.random.default_rng(M * 100003 + K)
    specials = {
        'zero': np.zeros(K, f16),
        'first': np.r_[f16(-7.5), (rng.standard_normal(K - 1) * 0.5).clip(-7, 7)].astype(f16),
        'last': np.r_[(rng.standard_normal(K - 1) * 0.5).clip(-7, 7), f16(9.25)].astype(f16),
        'extreme': np.r_[rng.standard_normal(5), 65504.0, rng.standard_normal(K - 9) * 100, -65504.0, rng.standard_normal(2)].astype(f16),
        'subnormal': (rng.integers(-1023, 1024, K) * 2.0**-24).astype(f16),
    }
    assert np.isfinite(specials['extreme'].astype(f32)).all() and np.abs(specials['extreme'].astype(f32)).max() >= 65000
    kinds = list(specials)
    for first in range(0, len(kinds), M):
        x = (rng.standard_normal((M, K)) * rng.uniform(0.01, 30.0, (M, 1))).astype(f16)
        for i, kind in enumerate(kinds[first:first + M]):
            x[(7 * i + 2) % M] = specials[kind]
        xq = torch.full((M + 1, K), 0xA5, dtype=torch.uint8, device='cuda')
        sx = torch.full((M + 1,), float('nan'), dtype=torch.float32, device='cuda')
        xd = dev(np.concatenate([x, np.full((1, K), np.nan, f16)]))
        _ffi.check(tm.tm_quant_fp8_token(xq.data_ptr(), sx.data_ptr(), xd.data_ptr(), K, M, K, st()))
        q_ref, s_ref = r.quant(x)
        got_q, got_s = host(xq), host(sx)
        assert np.array_equal(got_s[:M].view(np.uint32), s_ref.view(np.uint32)), 'activation scales must be bit exact'
        assert np.array_equal(got_q[:M], q_ref), f'{int((got_q[:M] != q_ref).sum())} codes differ'
        assert (got_q[M] == 0xA5).all() and np.isnan(got_s[M]), 'the row behind the last one was written'


# ---- (ii) the GEMM on exactly summable operands -----------------------------------------------------------------------------
@pytest.mark.parametrize('K,N,gated', [(128, 96, False), (640, 96, False), (128, 256, True), (640, 256, True)])
def test_linear_exact(tm, cuda, K, N, gated):
    """bit for bit at K = 128 (one k-block, one stage) and 640 (five k-blocks: the odd tail stage), N = 96 (three column groups
    under CG = 4) and 256 gated, M over both tile forms and a second row block with one live row, splits 0 (heuristic) .. 3"""
    wq, sw, pivot = r.exact_weight(K, N, gated)
    lin = _Linear(tm, wq, sw)
    try:
        for M in (1, 33, 64, 65, 130):
            x = r.exact_x(M, K, pivot, gated)
            want = r.assert_exactly_summable(x, wq, sw, gated)
            for splits in (0, 1, 2, 3):
                if splits > 1 and K < 256 * splits // 2:
                    continue
                got = lin(x, gated, splits)
                bad = _bits(got) != _bits(want)
                assert not bad.any(), (f'M {M} splits {splits}: {int(bad.sum())} outputs differ, first at {np.argwhere(bad)[0].tolist()}: '
                                       f'got {got[tuple(np.argwhere(bad)[0])]!r} want {want[tuple(np.argwhere(bad)[0])]!r}')
    finally:
        lin.close()


# ---- (iii) random operands ----------------------------------------------------------------------------------------------------
def _random_weight(rng, K, N):
    w = rng.standard_normal((K, N)) * (0.1 / np.sqrt(K)) * rng.uniform(0.25, 4.0, (1, N))
    sw = (np.abs(w).max(axis=0) / 448.0).astype(f32)
    wq = o.fp8_e4m3_from_f32(w / sw)
    wq[::37, ::11] = 0x01
    wq[5::53, 3::7] = 0xFE
    return wq, sw


@pytest.mark.parametrize('K,N', [(512, 256), (384, 64)])
def test_linear_random(tm, cuda, K, N):
    """both sides contract the same codes, so only the order of accumulation differs: the block-scaled test's bounds,
    2e-3 + 2^-9 |ref| plain and 2e-3 + 2^-8 |ref| gated"""
    rng = np.random.default_rng(K * 3 + N)
    wq, sw = _random_weight(rng, K, N)
    lin = _Linear(tm, wq, sw)
    try:
        for M in (1, 17, 64, 130):
            x = (rng.standard_normal((M, K)) * rng.uniform(0.2, 4.0, (M, 1))).astype(f16)
            for gated in (False, True):
                ref = r.linear(x, wq, sw, gated).astype(f32)
                for splits in (0, 1, 2):
                    err = np.abs(lin(x, gated, splits).astype(f32) - ref)
                    print(f'K {K} N {N} M {M} gated {gated} splits {splits}: max err {err.max():.3e}')
                    assert np.all(err <= 2e-3 + 2.0**(-8 if gated else -9) * np.abs(ref)), f'M={M} gated={gated} splits={splits}: {err.max()}'
    finally:
        lin.close()


# ---- (iv) grouped -----------------------------------------------------------------------------------------------------------------
SEG = np.array([0, 5, 5, 38, 45], np.int32)                     # 4 experts: 5 rows, none, 33, 7


def _run_grouped(tm, handles, x, gated, row_idx, rows):
    E, K, T = len(handles), x.shape[1], x.shape[0]
    N = handles[0].N
    ldy, F = (N // 2 if gated else N), int(SEG[-1])
    arr = (_ffi.C.c_void_p * E)(*[h.h for h in handles])
    ws = torch.full((tm.tm_linear_fp8_grouped_workspace(E, T, K),), 0xFF, dtype=torch.uint8, device='cuda')
    y = torch.full((F + 1, ldy), SENT, dtype=torch.int16, device='cuda').view(torch.float16)
    _ffi.check(tm.tm_debug_set_grouped_rows(rows))
    try:
        _ffi.check(tm.tm_linear_forward_fp8_grouped(arr, E, dev(x).data_ptr(), K, T, y.data_ptr(), ldy, 40, int(gated), dev(SEG).data_ptr(),
                                                    None if row_idx is None else dev(row_idx).data_ptr(), ws.data_ptr(), st()))
        torch.cuda.synchronize()
    finally:
        tm.tm_debug_set_grouped_rows(0)
    got = host(y)
    assert (got[F].view(np.uint16) == SENT).all(), 'the row behind the last one was written'
    return got[:F]


@pytest.mark.parametrize('gated', [False, True], ids=['plain', 'gated'])
def test_grouped(tm, cuda, gated):
    """4 experts (one without rows, one with 33: a second 32-row block with one live row), x rows gathered through row_idx and
    taken in place, 32- and 64-row tiles: the exact operands bit for bit, random operands within (iii)'s bounds"""
    K, N, F = 640, 256, int(SEG[-1])
    rng = np.random.default_rng(99 + gated)
    T = 20
    row_idx = rng.integers(0, T, F).astype(np.int32)
    # exact: one pivot for all experts' weights (the +448 element of x must meet a code >= 1 in every expert's gate columns)
    exact, pivot = [], None
    for e in range(4):
        wq, sw, pv = r.exact_weight(K, N, gated, seed=e)
        if pivot is None:
            pivot = pv
        elif gated:
            wq = wq.copy()
            wq[[pivot, pv]] = wq[[pv, pivot]]
        exact.append((wq, sw))
    rnd = [_random_weight(rng, K, N) for _ in range(4)]
    for name, experts in (('exact', exact), ('random', rnd)):
        handles = [_Linear(tm, wq, sw) for wq, sw in experts]
        try:
            for gather in (True, False):
                rows_x = T if gather else F
                if name == 'exact':
                    x = r.exact_x(rows_x, K, pivot, gated, seed=3)
                    for wq, sw in experts:
                        r.assert_exactly_summable(x, wq, sw, gated)
                else:
                    x = (rng.standard_normal((rows_x, K)) * rng.uniform(0.2, 4.0, (rows_x, 1))).astype(f16)
                ri = row_idx if gather else None
                want = r.grouped(x, experts, SEG, ri, gated)
                for rows in (32, 64):
                    got = _run_grouped(tm, handles, x, gated, ri, rows)
                    what = f'{name} gather {gather} rows {rows}'
                    if name == 'exact':
                        bad = _bits(got) != _bits(want)
                        assert not bad.any(), f'{what}: {int(bad.sum())} outputs differ, first at flat row, column {np.argwhere(bad)[0].tolist()}'
                    else:
                        ref = want.astype(f32)
                        err = np.abs(got.astype(f32) - ref)
                        assert np.all(err <= 2e-3 + 2.0**(-8 if gated else -9) * np.abs(ref)), f'{what}: max err {err.max()}'
        finally:
            for h in handles:
                h.close()


def test_weight_only_path_is_refused(tm, cuda, monkeypatch):
    """TM_FP8_MFMA=0 is not offered for channel-scaled weights: the preparation refuses and says why; tm_linear_forward (the
    weight-only kernel) refuses a weight prepared for the matrix cores"""
    wq, sw, _ = r.exact_weight(128, 96)
    lin = _Linear(tm, wq, sw)
    try:
        y = torch.zeros((1, 96), dtype=torch.float16, device='cuda')
        rc = tm.tm_linear_forward(lin.h, dev(np.zeros((1, 128), f16)).data_ptr(), 128, y.data_ptr(), 96, 1, 0, 0, 0, 0, None, st())
        assert rc != 0 and 'weight-only' in tm.tm_last_error().decode()
    finally:
        lin.close()
    monkeypatch.setenv('TM_FP8_MFMA', '0')
    h = _ffi.C.c_void_p()
    _ffi.check(tm.tm_linear_create(_ffi.C.byref(h), 128, 96, 2, 128))
    try:
        rc = tm.tm_linear_prepare_fp8_channel(h, dev(wq).data_ptr(), dev(sw).data_ptr(), st())
        assert rc != 0 and 'subnormal' in tm.tm_last_error().decode()
    finally:
        tm.tm_linear_destroy(h)


# ---- (v) engine and pipeline --------------------------------------------------------------------------------------------------------
TOYS = {
    'dense': dict(dialect='fp8', strategy='tensor'),
    'dense-d64': dict(dialect='compressed-tensors', strategy='channel', head_dim=64, q_heads=4, kv_heads=2, static=True),
    'mixtral': dict(dialect='compressed-tensors', strategy='channel', experts=4, top_k=2, inter=256),
}
PROMPT_LENS = (70, 9, 33)
STEPS = 3
_CKPT, _REF = {}, {}


def _toy(tmp_path_factory, name):
    """(path, what was written): one checkpoint per toy and session"""
    if name not in _CKPT:
        path = str(tmp_path_factory.mktemp('fp8ch_' + name))
        _CKPT[name] = (path, r.write_checkpoint(path, seed=11, **TOYS[name]))
    return _CKPT[name]


def _reference(name, ck, kv_bits, prompts, toks):
    """logits and residual stream of the reference model, teacher-forced with the engine's tokens; computed once per token path"""
    key = (name, kv_bits, toks.tobytes())
    if key not in _REF:
        oc = r.oracle_config(ck, kv_bits)
        om = r.ChannelModel(oc, r.tm_weights(ck, oc), batch=len(prompts), max_ctx=128)
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
    """toy checkpoints (per-tensor AutoFP8 dialect; per-channel compressed-tensors with head_dim 64 and static scales to read past;
    a per-channel Mixtral) -> read_config / load_hf_weights -> Engine: a prefill of ragged prompts (two forwards of <= 96 tokens)
    and 3 decode steps against ChannelModel on weights assembled by the reference module.  Bounds: the block-fp8 engine tests'
    3e-2 on the logits (tests/test_gpu_engine.py, fmt='fp8'), 2e-2 on the residual stream of the decode steps (tests/test_gpu_tp.py)"""
    from lmdeploy_amd.turbomind import checkpoint
    from lmdeploy_amd.turbomind.engine import Engine
    from lmdeploy_amd.turbomind.loader import export_weights
    path, ck = _toy(tmp_path_factory, name)
    cfg = checkpoint.read_config(path)
    assert cfg.weight_format == 'fp8' and cfg.fp8_scale_mode == 1 and cfg.head_dim == TOYS[name].get('head_dim', 128)
    rng = np.random.default_rng(3)
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in PROMPT_LENS]
    eng = Engine.from_model_config(cfg, weight_type=2, max_batch_size=len(prompts), session_len=128, quant_policy=quant_policy,
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
    for s in range(STEPS + 1):
        d = np.abs(logits[s].astype(f32) - ref_logits[s].astype(f32)).max()
        dr = np.abs(resid[s].astype(f32) - ref_resid[s].astype(f32)).max() if s else 0.0
        print(f'{name} qp {quant_policy} graph {use_graph} step {s}: max logit diff {d:.4g}, max residual diff {dr:.4g}')
        assert d <= 3e-2, f'step {s}: max logit diff {d}'
        assert dr <= 2e-2, f'step {s}: max residual diff {dr}'


def test_checkpoint_through_pipeline(cuda, tmp_path_factory):
    """the per-tensor toy through pipeline(path): greedy tokens and first-step logits against ChannelModel"""
    from lmdeploy_amd import GenerationConfig, TurbomindEngineConfig, pipeline
    path, ck = _toy(tmp_path_factory, 'dense')
    rng = np.random.default_rng(21)
    prompts = [rng.integers(3, 512, n).astype(np.int32).tolist() for n in (19, 5, 40)]
    N = 4
    pipe = pipeline(path, backend_config=TurbomindEngineConfig(model_format='fp8_channel', quant_policy=8, max_batch_size=3, session_len=128))
    try:
        assert pipe.model_cfg.fp8_scale_mode == 1
        got = [x.token_ids for x in pipe(prompts, GenerationConfig(max_new_tokens=N, ignore_eos=True))]
        pipe.engine.prefill(prompts, max_new_tokens=2)
        lg0 = pipe.engine.fetch_logits().astype(f32)
        pipe.engine.release()
    finally:
        pipe.close()
    oc = r.oracle_config(ck, 8)
    om = r.ChannelModel(oc, r.tm_weights(ck, oc), batch=3, max_ctx=128)
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


def test_synthetic_channel_engine_runs(cuda):
    """tm_engine_init_synthetic fills channel-mode slots with usable values: finite logits that differ between prompts, dense and MoE;
    stats() counts every linear's codes and column scales (K N + 4 N) next to the fp16 lm_head"""
    from lmdeploy_amd import GenerationConfig, TurbomindEngineConfig, pipeline
    from tests.linear_bytes import engine_weight_bytes
    for model in ('synthetic:tiny', 'synthetic:tiny_moe'):
        pipe = pipeline(model, backend_config=TurbomindEngineConfig(model_format='fp8_channel', quant_policy=8, max_batch_size=2, session_len=128))
        try:
            assert pipe.engine.stats()['weight_bytes'] == engine_weight_bytes(pipe.model_cfg, 'fp8_channel')
            out = pipe([[1, 2, 3, 4, 5], [9, 8, 7]], GenerationConfig(max_new_tokens=3, ignore_eos=True, output_logits='generation'))
            lg = np.stack([x.logits for x in out]).astype(f32)
            assert np.isfinite(lg).all() and lg.std() > 1e-3 and not np.array_equal(lg[0], lg[1])
        finally:
            pipe.close()
