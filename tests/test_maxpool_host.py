"""The stem MaxPool2d of the RGB ResNet-18 trunks (reference models/backbone.py:252-259) on the host: model rows, import rules,
checkpoint mapping, the compiled op against the numpy interpreter (oracle/circuit_ref.py), blob validation, noise budget and
bootstrap counts (no GPU)."""
import hashlib
import struct
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

GEOMS = [((3, 2, 1), 9), ((7, 4, 1), 13), ((2, 2, 0), 8), ((3, 1, 1), 6), ((3, 2, 1), 7), ((2, 2, 0), 9)]   # last two: odd H / W


@pytest.mark.parametrize("img,pool,feat_side", [(128, (3, 2, 1), 1), (224, (3, 2, 1), 1), (448, (3, 2, 1), 1), (1024, (7, 4, 1), 1)])
def test_resnet18_rgb_rows_build(img, pool, feat_side):
    from dctfhe import models
    m = models.ResNet18QAT(in_channels=3, img_size=img)
    assert m.pool1 == pool and m.conv1.weight.shape == (64, 3, 7, 7) and (m.conv1.stride, m.conv1.pad) == (2, 3)
    assert m.final_feat_dim == 512 * feat_side ** 2
    s = models.pool_out((img + 6 - 7) // 2 + 1, pool)
    for b in m.blocks:
        s = (s + 2 - 3) // b.C1.stride + 1
    assert s // m.avgpool_kernel == feat_side and m.classifier_w.shape == (10, m.final_feat_dim)


def test_existing_rows_keep_no_pool():
    from dctfhe import models
    assert models.ResNet18QAT(in_channels=48, img_size=112).pool1 is None and models.ResNet20QAT(in_channels=24, img_size=16).pool1 is None
    assert models.tiny_resnet_q().pool1 is None


class _Block(nn.Module):          # the SimpleBlock shape the importer reads (C1, BN1, C2, BN2)
    def __init__(self, c):
        super().__init__()
        self.C1, self.BN1 = nn.Conv2d(c, c, 3, 1, 1, bias=False), nn.BatchNorm2d(c)
        self.C2, self.BN2 = nn.Conv2d(c, c, 3, 1, 1, bias=False), nn.BatchNorm2d(c)

    def forward(self, x):
        return F.relu(self.BN2(self.C2(F.relu(self.BN1(self.C1(x))))) + x)


def _trunk(*mid, after=()):
    return nn.Sequential(nn.Identity(), nn.Conv2d(3, 8, 7, 2, 3, bias=False), nn.BatchNorm2d(8), *mid, _Block(8), *after, nn.AvgPool2d(2),
                         nn.Identity(), nn.Flatten())


def test_pooled_twin_imports_and_matches_torch():
    from dctfhe import models
    from dctfhe.torch_import import from_torch_module, seed_parameters
    net = seed_parameters(_trunk(nn.ReLU(), nn.MaxPool2d(3, 2, 1), nn.Identity()), 3).eval().double()
    m = from_torch_module(net, img_size=32)
    assert m.pool1 == (3, 2, 1) and m.relu1
    assert m.final_feat_dim == 8 * (((32 + 6 - 7) // 2 + 1 + 2 - 3) // 2 + 1) ** 2 // 4
    x = np.random.default_rng(0).normal(0, 1, (2, 3, 32, 32))
    with torch.no_grad():
        want = net(torch.from_numpy(x)).numpy()
    assert np.allclose(models.float_forward(m, x), want, atol=1e-9)


@pytest.mark.parametrize("layers", [
    dict(mid=(nn.MaxPool2d(3, 2, 1), nn.ReLU())),                                 # before the ReLU
    dict(mid=(nn.ReLU(),), after=(nn.MaxPool2d(3, 2, 1),)),                       # after a block
    dict(mid=(nn.ReLU(), nn.MaxPool2d(3, 2, 1), nn.MaxPool2d(3, 2, 1))),         # twice
    dict(mid=(nn.ReLU(), nn.MaxPool2d((3, 2), 2, 1))),                            # not square
    dict(mid=(nn.ReLU(), nn.MaxPool2d(3, 2, 1, dilation=2))),
    dict(mid=(nn.ReLU(), nn.MaxPool2d(3, 2, 1, ceil_mode=True))),
    dict(mid=(nn.ReLU(), nn.MaxPool2d(3, 2, 1, return_indices=True))),
])
def test_other_pool_placements_are_refused(layers):
    from dctfhe.torch_import import from_torch_module
    with pytest.raises(ValueError, match="MaxPool2d"):
        from_torch_module(_trunk(*layers["mid"], after=layers.get("after", ())))


def test_checkpoint_with_pool_maps_stem_scales(tmp_path):
    """a reference-layout best.tar whose trunk is [quant_inp, conv1, bn1, relu, pool1, quant_out, blocks..]: the pool has no parameters,
    the activation scales still land on stem_relu / stem_quant_out"""
    from dctfhe import checkpoint, models
    model = models.tiny_resnet_q(in_channels=3, img_size=9, pool1=(3, 2, 1))
    rng = np.random.default_rng(0)
    AQ = "act_quant.fused_activation_quant_proxy.tensor_quant.scaling_impl.value"
    st = {}
    T = "module.feature.trunk."

    def bn(name, c):
        for f, v in (("weight", rng.uniform(.5, 1.5, c)), ("bias", rng.normal(0, .1, c)), ("running_mean", rng.normal(0, 1, c)),
                     ("running_var", rng.uniform(.5, 2, c))):
            st[f"{T}{name}.{f}"] = torch.from_numpy(v).float()
    st[T + "1.weight"] = torch.from_numpy(rng.normal(0, .1, model.conv1.weight.shape)).float()
    bn("2", model.conv1.weight.shape[0])
    st[f"{T}0.{AQ}"], st[f"{T}3.{AQ}"], st[f"{T}5.{AQ}"] = torch.tensor(2.0), torch.tensor(3.0), torch.tensor([1.6])
    for i, b in enumerate(model.blocks):
        n = 6 + i
        st[f"{T}{n}.C1.weight"] = torch.from_numpy(rng.normal(0, .1, b.C1.weight.shape)).float()
        st[f"{T}{n}.C2.weight"] = torch.from_numpy(rng.normal(0, .1, b.C2.weight.shape)).float()
        bn(f"{n}.BN1", b.C1.weight.shape[0]); bn(f"{n}.BN2", b.C2.weight.shape[0])
        if b.shortcut is not None:
            st[f"{T}{n}.shortcut.weight"] = torch.from_numpy(rng.normal(0, .1, b.shortcut.weight.shape)).float()
            bn(f"{n}.BNshortcut", b.shortcut.weight.shape[0])
    st[f"{T}{6 + len(model.blocks) + 1}.{AQ}"] = torch.tensor(0.8)
    path = str(tmp_path / "best.tar")
    torch.save({"state": st}, path)
    _, unused = checkpoint.load_checkpoint(path, model)
    a = model.act_scales
    near = lambda x, y: abs(x - y) < 1e-7
    assert unused == [] and near(a["quant_inp"], 2.0 / 8) and near(a["stem_relu"], 3.0 / 15) and near(a["stem_quant_out"], 1.6 / 8)
    assert near(a["final"], 0.8 / 8)


def _pooled(pool, img, bits=4):
    from dctfhe import compile as cc, models, params as P
    calib = np.random.default_rng(1).normal(0, 1, (24, 4, img, img))
    return cc.compile_model(models.tiny_resnet_q(img_size=img, pool1=pool, bit_width=bits), calib, n_bits=5, param_set=P.test_params()), calib


@pytest.mark.parametrize("pool,img", GEOMS)
def test_compiled_pool_matches_numpy(pool, img):
    from dctfhe import compile as cc
    from oracle import circuit_ref as mref
    c, calib = _pooled(pool, img)
    ops = [o for o in c.ops if o.type == cc.OP_MAXPOOL]
    assert len(ops) == 1
    o = ops[0]
    assert list(o.ip[:3]) == list(pool) and o.ip[5] == 5 and o.payload.size == 32
    q = cc.act_quant(calib, c.in_scale, True, c.in_bits)
    ph = (q.astype(np.int64).astype(np.uint64) << np.uint64(c.e_in)).reshape(q.shape[0], -1)
    vals, overflow = mref.run_clear(c.blob, ph, all_tensors=True)
    assert not overflow
    e = c.tensors[o.src0].e
    assert c.tensors[o.dst].e == e
    x = (vals[o.src0].view(np.int64) >> np.int64(e))
    y = (vals[o.dst].view(np.int64) >> np.int64(e))
    assert x.min() >= 0 and x.max() <= 15 and len(np.unique(x)) > 3
    assert np.array_equal(y, F.max_pool2d(torch.from_numpy(x.astype(np.float64)), *pool).numpy().astype(np.int64))
    assert np.array_equal(y, cc.max_pool_int(x, *pool))
    # the relu table of the pairwise maxima: relu(d) at the tensor's encoding over the signed 5-bit differences
    assert np.array_equal(o.payload.ravel().view(np.uint64), np.maximum(np.arange(32) - 16, 0).astype(np.uint64) << np.uint64(e))
    # pairwise maxima = sum of (taps - 1) over both passes
    H = c.tensors[o.src0].H
    Wo = c.tensors[o.dst].W
    taps = cc.pool_taps(H, *pool)
    assert o.n_max == c.tensors[o.src0].C * (H * sum(t - 1 for t in taps) + Wo * sum(t - 1 for t in taps))
    # ... and the circuit's output is a valid signed 4-bit tensor
    out = vals[c.output_tensor].view(np.int64) >> np.int64(c.e_out)
    assert out.min() >= -8 and out.max() <= 7
    assert "max_pool2d(" in c.report()


@pytest.fixture(scope="module")
def L():
    from dctfhe import _lib
    return _lib.load()


def _rec(c, idx):
    nT = len(c.tensors)
    return 32 + 16 * nT + 96 * idx


@pytest.mark.parametrize("pool,img", GEOMS)
def test_validator_accepts_pooled_blobs(L, pool, img):
    c, _ = _pooled(pool, img)
    assert L.dctfhe_circuit_validate(c.blob, len(c.blob)) == 0, L.dctfhe_last_error().decode()


def test_validator_rejects_bad_pool_records(L):
    from dctfhe import compile as cc
    c, _ = _pooled((3, 2, 1), 9)
    i = next(j for j, o in enumerate(c.ops) if o.type == cc.OP_MAXPOOL)
    base = _rec(c, i)

    def bad(field_off, fmt, val, needle):
        b = bytearray(c.blob)
        struct.pack_into(fmt, b, base + field_off, val)
        assert L.dctfhe_circuit_validate(bytes(b), len(b)) != 0
        assert needle in L.dctfhe_last_error().decode(), L.dctfhe_last_error().decode()
    ip = lambda j: 16 + 4 * j
    bad(ip(0), "<i", 0, "bad max-pool geometry")            # k
    bad(ip(1), "<i", 0, "bad max-pool geometry")            # stride
    bad(ip(2), "<i", 2, "bad max-pool geometry")            # padding > k/2
    bad(ip(2), "<i", -1, "bad max-pool geometry")
    bad(ip(1), "<i", 1, "max-pool output shape mismatch")   # another stride, the recorded output
    bad(ip(5), "<i", 6, "max-pool table payload")           # p_d disagrees with the table
    bad(ip(5), "<i", 1, "bad max-pool difference precision")
    bad(ip(3), "<i", 60, "bad max-pool difference precision")
    bad(ip(4), "<i", 99, "max-pool tier")
    bad(88, "<q", 8 * 31, "max-pool table payload")
    # the output tensor with another channel count
    o = c.ops[i]
    b = bytearray(c.blob)
    struct.pack_into("<i", b, 32 + 16 * o.dst, c.tensors[o.dst].C + 1)
    assert L.dctfhe_circuit_validate(bytes(b), len(b)) != 0 and "channel count" in L.dctfhe_last_error().decode()


def test_pbs_counts_include_the_pool():
    from dctfhe import compile as cc
    c, _ = _pooled((3, 2, 1), 9)
    got = c.pbs_counts()
    o = next(o for o in c.ops if o.type == cc.OP_MAXPOOL)
    assert o.n_max > 0 and got[c.param_set.tiers[o.ip[4]].name] >= o.n_max


@pytest.mark.parametrize("bits", [4, 5])
def test_resnet18_224_circuit(bits):
    from dctfhe import compile as cc, models
    m = models.ResNet18QAT(bit_width=bits, in_channels=3, img_size=224)
    calib = np.random.default_rng(0).normal(0, 1, (2, 3, 224, 224))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        c = cc.compile_model(m, calib)
    o = next(o for o in c.ops if o.type == cc.OP_MAXPOOL)
    assert list(o.ip[:3]) == [3, 2, 1] and o.ip[5] == bits + 1 and o.n_max == 1193472
    assert c.tensors[o.src0].C * c.tensors[o.src0].H * c.tensors[o.src0].W == 802816
    tier = c.param_set.tiers[o.ip[4]].name
    if bits == 4:
        # exact budget met: no warning; the pool's 1 193 472 bootstraps in the counts, on the 5-bit coarse tier
        assert not [x for x in w if "budget" in str(x.message)]
        assert c.worst_site_failure <= 1e-12 and o.pfail < 1e-15
        assert tier == "T5a" and c.pbs_counts()[tier] >= 1193472
        # the stem's first table feeds the pool through the split + refresh path: the pool reads rows of 2048 mask words
        assert c.tensors[o.src0].deff == 2048 and c.tensors[o.dst].deff == 4096
        assert "max_pool2d(" in c.report()
    else:
        # p_d = 6 on the 6-bit coarse tier; the parent catalogue's 5-bit residual blocks exceed the exact budget on their own
        assert tier == "T6a" and c.pbs_counts()[tier] >= 1193472


PARENT_BLOBS = {    # compile_model of the four bench configurations, seeded weights (seed 1) and calibration (seed 7), on the parent commit
    "r20_24_16": "06166c110d0f9f42407e3fc5020560257862a181b4dfd195e863cc5a84b91748",
    "r20_3_32": "cca1a7e8a00e2ee2aac8e2c382e6988246dedefc922c44b134684e251ee237ba",
    "r18_3_32": "2446a8580ef336f6c87b1838a0e799402eca8764344149e936eeedee3f946265",
    "r18_48_112": "71292e3605b20302f293691ee77d88a74353e6b4c795219f2001b6c21bb09469",
}


@pytest.mark.parametrize("name,fac,cin,img", [("r20_24_16", "ResNet20QAT", 24, 16), ("r20_3_32", "ResNet20QAT", 3, 32),
                                              ("r18_3_32", "ResNet18QAT", 3, 32), ("r18_48_112", "ResNet18QAT", 48, 112)])
def test_pool_free_blobs_unchanged(name, fac, cin, img):
    from dctfhe import compile as cc, models
    m = getattr(models, fac)(in_channels=cin, img_size=img, seed=1)
    calib = np.random.default_rng(7).normal(0, 1, (4, cin, img, img))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert hashlib.sha256(cc.compile_model(m, calib).blob).hexdigest() == PARENT_BLOBS[name]
