"""MXFP4 W4A4 dense linears on the GPU against tests/mxfp4_dense_reference.py, through the C-ABI: the activation quantiser bit for
bit over every finite fp16 pattern, the repack through tm_linear_dequant_f16, the block-scaled FP4 MFMA GEMM bit for bit on exactly
summable operands and within a derived bound on random ones, the refusals, then a toy Quark checkpoint through Engine / pipeline()."""
import numpy as np
import pytest
import torch

from lmdeploy_amd import _ffi
from tests import mxfp4_dense_reference as r
from tests.gpu_helpers import dev, host, st

pytestmark = pytest.mark.gpu
f16, f32 = np.float16, np.float32
SENT = 0x7DAD                                                   # an fp16 NaN pattern no kernel writes


def _bits(a):
    """uint16 view with -0 mapped to +0"""
    v = np.ascontiguousarray(a, f16).view(np.uint16).copy()
    v[v == 0x8000] = 0
    return v


def _quant(tm, x, ldx=None):
    """codes and scale bytes of x [M][K] laid out with row stride ldx; the row behind the last one must stay poisoned"""
    M, K = x.shape
    ldx = ldx or K
    xp = np.full((M + 1, ldx), np.nan, f16)
    xp[:M, :K] = x
    xq = torch.full((M + 1, K // 2), 0xA5, dtype=torch.uint8, device='cuda')
    sx = torch.full((M + 1, K // 32), 0xA5, dtype=torch.uint8, device='cuda')
    _ffi.check(tm.tm_quant_mxfp4_rows(xq.data_ptr(), sx.data_ptr(), dev(xp).data_ptr(), ldx, M, K, st()))
    q, s = host(xq), host(sx)
    assert (q[M] == 0xA5).all() and (s[M] == 0xA5).all(), 'the row behind the last one was written'
    return q[:M], s[:M]


def _assert_quant(tm, x, ldx=None, what=''):
    q, s = _quant(tm, x, ldx)
    q_ref, s_ref = r.quant(x)
    bad = s != s_ref
    assert not bad.any(), f'{what}: {int(bad.sum())} scale bytes differ, first at {np.argwhere(bad)[0].tolist()}'
    bad = r.unpack_codes(q) != r.unpack_codes(q_ref)
    if bad.any():
        m, k = np.argwhere(bad)[0]
        raise AssertionError(f'{what}: {int(bad.sum())} codes differ, first at {(m, k)}: x {x[m, k]!r} (bits {int(x[m, k].view(np.uint16)):#06x}), '
                             f'scale byte {s_ref[m, k // 32]}, got {r.unpack_codes(q)[m, k]} want {r.unpack_codes(q_ref)[m, k]}')


# ---- (1) the quantiser ------------------------------------------------------------------------------------------------------
def test_quant_every_fp16_pattern(tm, cuda):
    """all finite fp16 patterns, each as the largest element of its group (the others at fixed fractions of it, down to zero) and
    as a non-largest element under a group maximum 1.5, 5 and 48 times its size (capped at the largest fp16), so that every
    pattern meets the scale of its own binade and of the binades above it: ties, saturation, subnormals and both zeros"""
    pat = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(f16)
    pat = pat[np.isfinite(pat.astype(f32))]
    assert pat.size == 63488
    frac = np.array([0.75, 0.5, 0.3, 0.125, 0.0, -0.6, -1.0, 0.9], np.float64)
    groups = []
    largest = np.zeros((pat.size, 32), np.float64)
    largest[:, 0] = pat.astype(np.float64)
    largest[:, 1:] = pat.astype(np.float64)[:, None] * np.resize(frac, 31)[None, :]
    groups.append(largest.astype(f16))
    groups[0][:, 0] = pat                                       # keeps -0
    for factor in (1.5, 5.0, 48.0):
        g = np.zeros((pat.size, 32), f16)
        g[:, 7] = pat
        g[:, 19] = np.minimum(np.abs(pat.astype(np.float64)) * factor, 65504.0).astype(f16)
        g[:, 20] = -g[:, 7]
        groups.append(g)
    x = np.concatenate(groups).reshape(-1, 128)
    _assert_quant(tm, x, what='every pattern')


@pytest.mark.parametrize('K', [128, 4224, 14336])
@pytest.mark.parametrize('M', [1, 3, 65])
def test_quant_rows_bit_exact(tm, cuda, M, K):
    """rows of very different magnitude with ldx > K; zero groups, groups of -0 / +0, fp16 extremes and subnormals"""
    rng = np.random.default_rng(M * 100003 + K)
    x = (rng.standard_normal((M, K)) * np.exp2(rng.integers(-12, 10, (M, K // 32))).repeat(32, axis=1)).astype(f16)
    x[0, :32] = 0
    x[M // 2, K - 32:] = np.where(np.arange(32) % 3 == 0, -0.0, 0.0).astype(f16)
    x[M - 1, 32:64] = (rng.integers(-1023, 1024, 32) * 2.0**-24).astype(f16)
    x[M - 1, 64:96] = np.r_[65504.0, -65504.0, rng.standard_normal(30) * 3e4].clip(-65504, 65504).astype(f16)
    assert np.isfinite(x.astype(f32)).all()
    _assert_quant(tm, x, ldx=K + 8, what=f'M {M} K {K}')


# ---- handles ----------------------------------------------------------------------------------------------------------------------
class _Linear:
    def __init__(self, tm, blocks, scales):
        self.tm, self.N, self.K = tm, blocks.shape[0], blocks.shape[1] * 2
        self.h = _ffi.C.c_void_p()
        _ffi.check(tm.tm_linear_create(_ffi.C.byref(self.h), self.K, self.N, 3, 32))
        _ffi.check(tm.tm_linear_prepare_mxfp4(self.h, dev(blocks).data_ptr(), dev(scales).data_ptr(), st()))
        torch.cuda.synchronize()

    def __call__(self, x, gated=False, splits=0):
        """y with one NaN-poisoned row behind the last one, which must come back untouched"""
        M, ldy = x.shape[0], self.N // 2 if gated else self.N
        ws = torch.full((self.tm.tm_linear_mxfp4_workspace(self.h, M),), 0xFF, dtype=torch.uint8, device='cuda')
        y = torch.full((M + 1, ldy), SENT, dtype=torch.int16, device='cuda').view(torch.float16)
        _ffi.check(self.tm.tm_linear_forward_mxfp4(self.h, dev(x).data_ptr(), self.K, y.data_ptr(), ldy, M, int(gated), splits,
                                                   ws.data_ptr(), st()))
        got = host(y)
        assert (got[M].view(np.uint16) == SENT).all(), 'the row behind the last one was written'
        return got[:M]

    def dequant(self):
        out = torch.full((self.N + 1, self.K), SENT, dtype=torch.int16, device='cuda').view(torch.float16)
        _ffi.check(self.tm.tm_linear_dequant_f16(self.h, out.data_ptr(), st()))
        got = host(out)
        assert (got[self.N].view(np.uint16) == SENT).all()
        return got[:self.N]

    def close(self):
        self.tm.tm_linear_destroy(self.h)


# ---- (2) the repack -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,N', [(128, 32), (640, 96)])
def test_repack_dequant_bit_exact(tm, cuda, K, N):
    """tm_linear_dequant_f16 rebuilds lut[code] * 2^(s - 127) from the repacked units, bit for bit, on a matrix whose groups run
    through all 37 scale bytes that keep every e2m1 value an fp16 (2^-23 .. 2^13) and hold all 16 codes each, rotated per group"""
    G = K // 32
    gi = np.arange(N * G).reshape(N, G)
    scales = (127 - 23 + gi % 37).astype(np.uint8)
    assert N * G >= 37
    codes = ((np.arange(32)[None, None, :] * 5 + gi[:, :, None] * 3) % 16).astype(np.uint8).reshape(N, K)
    assert all(len(set(row)) == 16 for row in codes.reshape(-1, 32))
    blocks = r.pack_codes(codes)
    want = r.dequant(blocks, scales)
    assert np.array_equal(want.astype(f16).astype(np.float64), want)
    lin = _Linear(tm, blocks, scales)
    try:
        got = lin.dequant()
    finally:
        lin.close()
    assert np.array_equal(got.view(np.uint16), want.astype(f16).view(np.uint16))


# ---- (3) the GEMM on exactly summable operands -----------------------------------------------------------------------------
@pytest.mark.parametrize('K,N,gated', [(128, 96, False), (640, 96, False), (128, 256, True), (640, 256, True), (4096, 64, False)])
def test_linear_exact(tm, cuda, K, N, gated):
    """bit for bit: K = 128 (one k-block), 640 (five: uneven k-phases and slices) and 4096, N = 96 / 64 (a partial workgroup of
    column groups) and 256 gated, M over the 32-, 64- and 128-row weight-streaming tiles and the 128-row prefill tile with a
    two-row tail, splits 0 (heuristic), 1, 2, 5 (slab reduction)"""
    blocks, scales = r.exact_weight(K, N, gated)
    lin = _Linear(tm, blocks, scales)
    try:
        for M in (1, 33, 65, 130):
            x = r.exact_x(M, K, gated)
            want = r.assert_exactly_summable(x, blocks, scales, gated)
            for splits in (0, 1, 2, 5):
                got = lin(x, gated, splits)
                bad = _bits(got) != _bits(want)
                assert not bad.any(), (f'M {M} splits {splits}: {int(bad.sum())} outputs differ, first at {np.argwhere(bad)[0].tolist()}: '
                                       f'got {got[tuple(np.argwhere(bad)[0])]!r} want {want[tuple(np.argwhere(bad)[0])]!r}')
    finally:
        lin.close()


# ---- (4) random operands ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,N', [(512, 256), (384, 64)])
def test_linear_random(tm, cuda, K, N):
    """against the float64 sum of the reference's own codes: |y - ref| <= 2^-11 |ref| + K 2^-24 sum_k |x_k w_k| -- one fp16 rounding
    plus the worst case of an fp32 chain of K terms; both derived, not tuned"""
    rng = np.random.default_rng(K * 3 + N)
    blocks, scales = r.quantize_weight(rng.standard_normal((N, K)) * (0.1 / np.sqrt(K)) * rng.uniform(0.25, 4.0, (N, 1)))
    lin = _Linear(tm, blocks, scales)
    try:
        M = 70
        x = (rng.standard_normal((M, K)) * rng.uniform(0.2, 4.0, (M, 1))).astype(f16)
        ref, mag = r.acc_f64(x, blocks, scales)
        for splits in (0, 2):
            err = np.abs(lin(x, False, splits).astype(np.float64) - ref)
            bound = 2.0**-11 * np.abs(ref) + K * 2.0**-24 * mag
            print(f'K {K} N {N} M {M} splits {splits}: max err {err.max():.3e}, max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}')
            assert np.all(err <= bound), f'splits {splits}: {int((err > bound).sum())} outputs beyond the bound, max err {err.max()}'
    finally:
        lin.close()


# ---- (5) refusals -----------------------------------------------------------------------------------------------------------------
def test_linear_refusals(tm, cuda):
    """tm_linear_forward has no weight-only arm for such a weight; K = 96 is refused with the limit named"""
    blocks, scales = r.exact_weight(128, 96)
    lin = _Linear(tm, blocks, scales)
    try:
        y = torch.zeros((1, 96), dtype=torch.float16, device='cuda')
        rc = tm.tm_linear_forward(lin.h, dev(np.zeros((1, 128), f16)).data_ptr(), 128, y.data_ptr(), 96, 1, 0, 0, 0, 0, None, st())
        assert rc == 1 and 'weight-only' in tm.tm_last_error().decode() and 'tm_linear_forward_mxfp4' in tm.tm_last_error().decode()
    finally:
        lin.close()
    h = _ffi.C.c_void_p()
    rc = tm.tm_linear_create(_ffi.C.byref(h), 96, 96, 3, 32)
    assert rc == 1 and 'K % 128 == 0' in tm.tm_last_error().decode()
    rc = tm.tm_linear_create(_ffi.C.byref(h), 128, 48, 3, 32)
    assert rc == 1 and 'N % 32 == 0' in tm.tm_last_error().decode()


def test_engine_refusals(cuda):
    """weight_type mxfp4 is a dense, single-rank format: an MoE model and tp = 2 are refused by name"""
    from lmdeploy_amd.turbomind.engine import Engine
    from oracle import tm_oracle as o
    kw = dict(hidden=256, layers=1, q_heads=2, kv_heads=2, head_dim=128, inter=256, vocab=512, rope=o.RopeParam(128, 10000.0, 'default', 1.0, 1.0, 4.0, 8192))
    with pytest.raises(Exception, match='moe_experts > 0'):
        Engine.from_model_config(o.ModelConfig(**kw, moe_experts=4, moe_top_k=2), weight_type=3, max_batch_size=2, session_len=128).close()
    with pytest.raises(Exception, match='tp > 1'):
        Engine.from_model_config(o.ModelConfig(**kw), weight_type=3, tp=2, rank=0, max_batch_size=2, session_len=128).close()


# ---- (6) engine and (7) pipeline ---------------------------------------------------------------------------------------------------
TOYS = {'d128': {}, 'd64': dict(head_dim=64, q_heads=4, kv_heads=2)}
PROMPT_LENS = (70, 9, 33)
STEPS = 3
_CKPT, _REF = {}, {}


def _toy(tmp_path_factory, name):
    """(path, what was written): one checkpoint per toy and session"""
    if name not in _CKPT:
        path = str(tmp_path_factory.mktemp('mxfp4_' + name))
        _CKPT[name] = (path, r.write_checkpoint(path, seed=11, **TOYS[name]))
    return _CKPT[name]


def _run_reference(ck, kv_bits, prompts, toks, perturb_seed=None):
    oc = r.oracle_config(ck, kv_bits)
    om = r.Mxfp4Model(oc, r.tm_weights(ck, oc), batch=len(prompts), max_ctx=128, perturb_seed=perturb_seed)
    logits = [om.forward(prompts)[1].astype(f32)]
    for s in range(STEPS):
        logits.append(om.forward([[int(t)] for t in toks[:, s]])[1].astype(f32))
    return logits


def _reference(name, ck, kv_bits, prompts, toks):
    """the reference's logits, teacher-forced with the engine's tokens, and S: the largest logit change over 8 reruns with every GEMM
    input perturbed by what the operator tests allow its producer; computed once per token path"""
    key = (name, kv_bits, toks.tobytes())
    if key not in _REF:
        logits = _run_reference(ck, kv_bits, prompts, toks)
        S = 0.0
        for seed in range(8):
            pert = _run_reference(ck, kv_bits, prompts, toks, perturb_seed=seed)
            S = max(S, max(float(np.abs(a - b).max()) for a, b in zip(pert, logits)))
        _REF[key] = (logits, S)
    return _REF[key]


@pytest.mark.parametrize('use_graph', [0, 1], ids=['eager', 'graph'])
@pytest.mark.parametrize('quant_policy', [0, 8])
@pytest.mark.parametrize('name', list(TOYS))
def test_engine_matches_reference(cuda, tmp_path_factory, name, quant_policy, use_graph):
    """the toy Quark checkpoint (hidden 256, 2 layers, inter 512; head_dim 128 and 64) -> read_config / load_hf_weights -> Engine:
    ragged prompts (70, 9, 33) under a 96-token prefill budget and 3 teacher-forced decode steps against Mxfp4Model.  FP4 activation
    codes are discontinuous -- one fp16 ulp upstream can flip a code --, so the logit bound is max(3e-2, 2 S): 3e-2 is the other
    formats' engine bound, S the reference's own sensitivity (printed; the factor 2 because 8 seeds under-sample a maximum)"""
    from lmdeploy_amd.turbomind import checkpoint
    from lmdeploy_amd.turbomind.engine import Engine
    from lmdeploy_amd.turbomind.loader import export_weights
    path, ck = _toy(tmp_path_factory, name)
    cfg = checkpoint.read_config(path)
    assert cfg.weight_format == 'mxfp4' and cfg.quantized and cfg.head_dim == TOYS[name].get('head_dim', 128)
    rng = np.random.default_rng(3)
    prompts = [rng.integers(0, cfg.vocab, n).astype(np.int32) for n in PROMPT_LENS]
    eng = Engine.from_model_config(cfg, weight_type=3, max_batch_size=len(prompts), session_len=128, quant_policy=quant_policy,
                                   max_prefill_token_num=96, use_graph=use_graph)
    try:
        eng.load_weights(export_weights(cfg, checkpoint.load_hf_weights(path, cfg)))
        eng.start()
        eng.prefill(prompts, max_new_tokens=STEPS + 1)
        logits = [eng.fetch_logits().copy()]
        for _ in range(STEPS):
            eng.decode(1)
            logits.append(eng.fetch_logits().copy())
        toks = eng.fetch()
    finally:
        eng.close()
    ref_logits, S = _reference(name, ck, 16 if quant_policy == 0 else quant_policy, prompts, toks)
    bound = max(3e-2, 2 * S)
    for s in range(STEPS + 1):
        d = np.abs(logits[s].astype(f32) - ref_logits[s]).max()
        print(f'{name} qp {quant_policy} graph {use_graph} step {s}: max logit diff {d:.4g} (S {S:.4g}, bound {bound:.4g})')
    for s in range(STEPS + 1):
        d = np.abs(logits[s].astype(f32) - ref_logits[s]).max()
        assert d <= bound, f'step {s}: max logit diff {d} > {bound} (S {S})'


def test_checkpoint_through_pipeline(cuda, tmp_path_factory):
    """the toy through pipeline(path, model_format='mxfp4', quant_policy=8): greedy tokens against Mxfp4Model with the top-2 margin rule"""
    from lmdeploy_amd import GenerationConfig, TurbomindEngineConfig, pipeline
    path, ck = _toy(tmp_path_factory, 'd128')
    rng = np.random.default_rng(21)
    prompts = [rng.integers(3, 512, n).astype(np.int32).tolist() for n in (19, 5, 40)]
    N = 4
    pipe = pipeline(path, backend_config=TurbomindEngineConfig(model_format='mxfp4', quant_policy=8, max_batch_size=3, session_len=128))
    try:
        assert pipe.model_cfg.weight_format == 'mxfp4'
        got = [x.token_ids for x in pipe(prompts, GenerationConfig(max_new_tokens=N, ignore_eos=True))]
    finally:
        pipe.close()
    oc = r.oracle_config(ck, 8)
    om = r.Mxfp4Model(oc, r.tm_weights(ck, oc), batch=3, max_ctx=128)
    _, ref = om.forward([np.asarray(p) for p in prompts])
    ref = ref.astype(f32)
    for s in range(N):
        for b in range(3):
            top = np.argsort(ref[b])[::-1][:2]
            margin = ref[b][top[0]] - ref[b][top[1]]
            assert got[b][s] == top[0] or (margin <= 6e-2 and got[b][s] == top[1]), (b, s, got[b][s], top, margin)
        if s + 1 < N:
            _, ref = om.forward([[got[b][s]] for b in range(3)])
            ref = ref.astype(f32)


def test_synthetic_engine_runs(cuda):
    """tm_engine_init_synthetic fills the blocks / scales slots with usable values: finite logits that differ between prompts;
    stats() counts every linear's codes and scale bytes (K N / 2 + N K / 32) next to the fp16 lm_head"""
    from lmdeploy_amd import GenerationConfig, TurbomindEngineConfig, pipeline
    from tests.linear_bytes import engine_weight_bytes
    pipe = pipeline('synthetic:tiny', backend_config=TurbomindEngineConfig(model_format='mxfp4', quant_policy=8, max_batch_size=2, session_len=128))
    try:
        assert pipe.engine.stats()['weight_bytes'] == engine_weight_bytes(pipe.model_cfg, 'mxfp4')
        out = pipe([[1, 2, 3, 4, 5], [9, 8, 7]], GenerationConfig(max_new_tokens=3, ignore_eos=True, output_logits='generation'))
        lg = np.stack([x.logits for x in out]).astype(f32)
        assert np.isfinite(lg).all() and lg.std() > 1e-3 and not np.array_equal(lg[0], lg[1])
    finally:
        pipe.close()
