"""The stem MaxPool2d (circuit op 5) on the GPU: the difference key switch, the pooling tree on encrypted rows and in clear mode,
pooled circuits against the numpy interpreter (oracle/circuit_ref.py), statistics, simulate, the CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import circuit_ref as mref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMS = [((3, 2, 1), 7, 9), ((7, 4, 1), 13, 13), ((2, 2, 0), 8, 9), ((3, 1, 1), 6, 5), ((2, 1, 1), 5, 4)]


@pytest.fixture(scope="module")
def keys(gpu_ctx):
    from dctfhe import params as P
    from dctfhe.engine import Keys
    ps = P.test_params()
    ps.input_dim = 512               # fresh encryptions mask 512 of the 1024 key words: inputs at a smaller effective dimension
    k = Keys(gpu_ctx, P.to_c_params(ps), seed=11)
    yield k
    k.close()


def _oracle(qm, q):
    ref, overflow = mref.run_clear(qm.compiled.blob, qm.encode_input(q))
    assert not overflow
    return qm.decode_output(ref)


def test_keyswitch_diff_equals_keyswitch_of_the_difference(keys):
    rng = np.random.default_rng(0)
    cts = keys.encrypt(rng.integers(0, 16, 40).astype(np.uint64) << np.uint64(58))
    assert cts[:, :512].any() and not cts[:, 512:1024].any()     # input_dim: the rows mask 512 of the 1024 key words
    # all 40 rows and 37 of them (not a multiple of the decompose kernel's 256-thread block), at full width and narrowed to the 512 words
    for n, deff in ((40, 0), (40, 512), (37, 0), (37, 512)):
        ia, ib = rng.integers(0, n, n).astype(np.int32), rng.integers(0, n, n).astype(np.int32)
        for tier in (0, 1):
            for shift, body_add in ((0, 1 << 62), (2, 0)):
                got = keys.keyswitch_diff(tier, cts[:n], ia, ib, shift, body_add, deff=deff)
                diff = cts[:n][ia] - cts[:n][ib]
                diff[:, -1] += np.uint64(body_add >> shift)          # body_add lands after the shift: pre-divide (exact for these values)
                want = keys.keyswitch(tier, diff, shift=shift, deff=deff)
                assert np.array_equal(got, want), (n, deff, tier, shift)


@pytest.mark.parametrize("pool,H,W", GEOMS)
def test_max_pool_rows_encrypted_and_clear(gpu_ctx, keys, pool, H, W):
    import torch
    import torch.nn.functional as F
    k, s, p = pool
    p_d, e = 5, 58
    rng = np.random.default_rng(k * 100 + H)
    v = rng.integers(0, 16, (2, 3, H, W))
    table = (np.maximum(np.arange(32) - 16, 0).astype(np.uint64) << np.uint64(e)).view(np.int64)
    want = F.max_pool2d(torch.from_numpy(v.astype(np.float64)), k, s, p).numpy().astype(np.int64)
    ph = (v.astype(np.uint64) << np.uint64(e))
    clear = gpu_ctx.max_pool_rows(ph, 0, k, s, p, p_d)
    assert np.array_equal(clear.view(np.int64) >> 58, want)
    assert np.array_equal(clear, mref.max_pool_words(ph, k, s, p))
    dim_in = 512                                                  # compact input rows; outputs at the table ring (1024)
    cts = keys.encrypt(ph.reshape(-1), dim_in).reshape(2, 3, H, W, dim_in + 1)
    out = gpu_ctx.max_pool_rows(cts, dim_in, k, s, p, p_d, table, 1024, keys=keys, tier=0)
    dec = keys.decrypt(out.reshape(-1, 1025), 1024).reshape(want.shape)
    got = ((dec + (np.uint64(1) << np.uint64(e - 1))) >> np.uint64(e)).astype(np.int64)
    assert np.array_equal(got, want), np.argwhere(got != want)


def test_max_pool_rows_refusals(gpu_ctx, keys):
    from dctfhe._lib import DctfheError
    x = np.zeros((1, 1, 4, 4), np.uint64)
    for k, s, p in ((0, 1, 0), (3, 0, 1), (3, 2, 2), (33, 1, 0), (5, 1, 0)):
        with pytest.raises(DctfheError, match="bad geometry"):
            gpu_ctx.max_pool_rows(x, 0, k, s, p, 5)
    with pytest.raises(DctfheError, match="p_d"):
        gpu_ctx.max_pool_rows(x, 0, 3, 2, 1, 40)
    cts = np.zeros((1, 1, 4, 4, 1025), np.uint64)
    table = np.zeros(32, np.int64)
    with pytest.raises(DctfheError, match="cannot hold"):
        gpu_ctx.max_pool_rows(cts, 1024, 3, 2, 1, 5, table, 512, keys=keys, tier=0)
    with pytest.raises(DctfheError, match="tier out of range"):
        gpu_ctx.max_pool_rows(cts, 1024, 3, 2, 1, 5, table, 1024, keys=keys, tier=7)
    with pytest.raises(DctfheError, match="does not fit"):
        gpu_ctx.max_pool_rows(cts, 1024, 3, 2, 1, 12, np.zeros(4096, np.int64), 1024, keys=keys, tier=1)
    with pytest.raises(DctfheError, match="out of range"):
        keys.keyswitch_diff(0, np.zeros((2, 1025), np.uint64), [0, 2], [1, 0])
    with pytest.raises(DctfheError, match="tier out of range"):
        keys.keyswitch_diff(5, np.zeros((2, 1025), np.uint64), [0, 1], [1, 0])


def _tiny_pooled(pool, img):
    from dctfhe import models, params as P
    from dctfhe.quantized_module import compile_brevitas_qat_model
    calib = np.random.default_rng(3).normal(0, 1, (24, 4, img, img))
    qm = compile_brevitas_qat_model(models.tiny_resnet_q(img_size=img, pool1=pool), calib[:20], n_bits=5, rounding_threshold_bits=6,
                                    param_set=P.test_params())
    return qm, calib


@pytest.mark.parametrize("pool,img", [((3, 2, 1), 9), ((2, 2, 0), 7)])
def test_tiny_pooled_trunk_encrypted_equals_interpreter(pool, img):
    from dctfhe import compile as cc
    qm, calib = _tiny_pooled(pool, img)
    try:
        q = qm.quantize_input(calib[20:23])
        want = _oracle(qm, q)
        assert np.array_equal(qm.forward_quantized(q, "disable"), want)
        qm.fhe_circuit.keygen(seed=5)
        got = qm.forward_quantized(q, "execute")
        assert np.array_equal(got, want), np.argwhere(got != want)
        # timing: bootstraps per tier of the run == the compiler's counts
        sess = qm._session("execute", 3)
        t = sess.run(timing=True)
        counts = qm.compiled.pbs_counts()
        names = [tt.name for tt in qm.compiled.param_set.tiers]
        assert {names[i]: t.pbs_cts[i] // 3 for i in range(len(names)) if t.pbs_cts[i]} == counts
        assert any(o.type == cc.OP_MAXPOOL for o in qm.compiled.ops)
        # simulate at the exact tiers == the clear circuit
        assert np.array_equal(qm.forward_quantized(q, "simulate"), want)
    finally:
        qm.close()


def _rgb(n, seed, size):
    from dctfhe import frontend, synthetic
    tf = frontend.rgb_eval_transform(size)
    return np.stack([tf(im) for im in synthetic.synthetic_images(n, seed)]).astype(np.float32)


def test_resnet18_224_all_stages_on_a_crop_encrypted():
    """the 64_3_224 model's weights and tiers, all four stages, on a 96x96 crop (avgpool 3): encrypted == interpreter, labels agree"""
    from dctfhe import models
    from dctfhe.quantized_module import compile_brevitas_qat_model
    x = _rgb(13, 7, 224)[:, :, 64:160, 64:160]
    model = models.ResNet18QAT(bit_width=4, in_channels=3, img_size=224)
    whole = models.trunk_prefix(model, n_blocks=8, avgpool_kernel=3)
    assert whole.pool1 == (3, 2, 1)
    qm = compile_brevitas_qat_model(whole, x[:12], n_bits=5, rounding_threshold_bits=6, p_error=0.01)
    try:
        q = qm.quantize_input(x[12:13])
        want = _oracle(qm, q)
        assert want.shape == (1, 512) and len(np.unique(want)) > 4
        qm.fhe_circuit.keygen(seed=1)
        got = qm.forward_quantized(q, "execute")
        assert np.array_equal(got, want), np.argwhere(got != want)
        cw = np.random.default_rng(0).normal(0, 1, (10, 512))
        assert (qm.dequantize_output(got) @ cw.T).argmax() == (qm.dequantize_output(want) @ cw.T).argmax()
    finally:
        qm.close()


def test_resnet18_224_full_size_clear_equals_interpreter():
    from dctfhe import models
    from dctfhe.quantized_module import compile_brevitas_qat_model
    x = _rgb(6, 9, 224)
    model = models.ResNet18QAT(bit_width=4, in_channels=3, img_size=224)
    # calibrated on the six images themselves: the accumulator ranges hold the two evaluated ones (four images alone may not)
    qm = compile_brevitas_qat_model(model, x, n_bits=5, rounding_threshold_bits=6, p_error=0.01)
    try:
        q = qm.quantize_input(x[4:6])
        want = _oracle(qm, q)
        assert np.array_equal(qm.forward_quantized(q, "disable"), want)
        assert np.array_equal(qm.forward_quantized(q, "simulate"), want)
        labels = (qm.dequantize_output(want) @ model.classifier_w.T).argmax(axis=1)
        assert labels.shape == (2,)
    finally:
        qm.close()


def test_cli_resnet18_224_disable():
    env = dict(os.environ)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "dct-cryptonets_amd", "homomorphic_eval.py"), "--model", "ResNet18qat", "--image_size",
                        "224", "--fhe_mode", "disable", "--test_subset", "2", "--verbose", ""],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Running ENCRYPTED test inference in DISABLE mode" in r.stdout and "Done" in r.stdout
