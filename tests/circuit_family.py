"""The committed, seeded family of small topologies that tests/test_circuit_family_host.py checks on the host and
tests/test_gpu_circuit_family.py runs on the device: stems, stem pools, block layouts, sum pools, rounding settings and channel counts
outside the one miniature (models.tiny_resnet_q) the rest of the suite builds on.  Every case compiles under params.test_params():
D = 1024, table tier `t` at N = 1024, bit tier `b` at k = 2, N = 256 -- rows at effective dimensions 512 and 1024 meet in one run.

A case is plain data: a model description built from ConvLayer / BatchNorm / QBlock with the reference initialisation and a fixed seed,
one draw of default_rng(seed) that holds the calibration batch first and the fresh inputs behind it, and the compile_model keywords.
Nothing is drawn at test time; a compiled case and the interpreter's outputs for it are computed once and shared, read-only."""
import functools
import math

import numpy as np

N_CALIB = 20
BATCH = 3                 # the largest batch a test of the family runs (ragged for every workgroup packing); batch 1 is its first image
BOUND = 1e-5              # expected failures per image x BATCH, for every case that is compared bit for bit


class Case:
    """stem = (cout, k, stride, pad); stages = [(cout, stride)]: one block each, a 1x1 shortcut where the width or the size changes;
    fresh: rows of the draw, behind the N_CALIB calibration rows, that the tests run -- chosen so that the integer circuit takes them
    without leaving a table's padded range (tests/test_circuit_family_host.py asserts it); kw: compile_model keywords"""

    def __init__(self, name, seed, in_ch, img, stem, stages, sum_k, relu1=True, pool1=None, bit_width=4, fresh=(20, 21, 22), **kw):
        self.name, self.seed, self.in_ch, self.img, self.stem, self.stages, self.sum_k = name, seed, in_ch, img, stem, list(stages), sum_k
        self.relu1, self.pool1, self.bit_width, self.fresh, self.kw = relu1, pool1, bit_width, tuple(fresh), kw
        assert len(self.fresh) == BATCH and min(self.fresh) >= N_CALIB

    exact = property(lambda s: s.kw.get("rounding_method", "exact") == "exact")

    def model(self):
        from dctfhe import models as M
        rng = np.random.default_rng(self.seed)
        c0, k0, s0, p0 = self.stem
        conv1 = M.ConvLayer(M._init_conv(rng, c0, self.in_ch, k0), s0, p0)
        size = M.pool_out((self.img + 2 * p0 - k0) // s0 + 1, self.pool1)
        blocks, indim = [], c0
        for outdim, stride in self.stages:
            b = M.QBlock(C1=M.ConvLayer(M._init_conv(rng, outdim, indim, 3), stride, 1), BN1=M._init_bn(outdim),
                         C2=M.ConvLayer(M._init_conv(rng, outdim, outdim, 3), 1, 1), BN2=M._init_bn(outdim))
            if indim != outdim or stride != 1:
                b.shortcut, b.BNshortcut = M.ConvLayer(M._init_conv(rng, outdim, indim, 1), stride, 0), M._init_bn(outdim)
            blocks.append(b)
            indim, size = outdim, (size + 2 - 3) // stride + 1
        feat = indim * (size // self.sum_k) ** 2
        return M.ResNetQ(name=self.name, in_channels=self.in_ch, img_size=self.img, bit_width=self.bit_width, conv1=conv1, bn1=M._init_bn(c0),
                         relu1=self.relu1, blocks=blocks, avgpool_kernel=self.sum_k, final_feat_dim=feat,
                         classifier_w=rng.normal(0, 1.0 / math.sqrt(feat), size=(10, feat)), classifier_b=np.zeros(10), pool1=self.pool1)

    def draw(self):
        """the case's one draw: rows [0, N_CALIB) calibrate, the rows named by `fresh` are run"""
        x = np.random.default_rng(self.seed + 1000).normal(0, 1, (max(self.fresh) + 1, self.in_ch, self.img, self.img))
        x.setflags(write=False)
        return x

    def calib(self):
        return self.draw()[:N_CALIB]

    def fresh_inputs(self):
        return self.draw()[list(self.fresh)]

    def compile_kw(self):
        from dctfhe import params as P
        return dict(self.kw, param_set=P.test_params())


# The first four are the shapes measured to meet the bound as they stand; the pool (3, 1, 1) trunk and the wide one are reshaped (below).
CASES = [
    # a signed stem table (relu1=False) behind a strided, padded 3x3 stem on an odd image (9 -> 5); one block, identity shortcut; the sum
    # pool drops a border row and column (5 // 2) and leaves 2 x 2; parity-split sites
    Case("signed-stem-s2", 1, 3, 9, (5, 3, 2, 1), [(5, 1)], 2, relu1=False, rounding_threshold_bits=7, n_bits=5),
    # 5x5 stem, MaxPool(2, 2, 0) on an odd size (11 -> 5, a row and a column unread), an identity block and a strided one whose 1x1
    # shortcut reads an odd size (5 -> 3); global sum pool
    Case("stem5-pool220", 2, 2, 11, (7, 5, 1, 2), [(7, 1), (9, 2)], 3, pool1=(2, 2, 0), rounding_threshold_bits=6, n_bits=5),
    # three stages, two of them strided, strided 1x1 shortcuts on even sizes (8 -> 4 -> 2); sum pool K = 1: 10 x 2 x 2 outputs.  With
    # four input channels this seed calibrates a 10-bit accumulator (four rounding steps: 1.2e-3 failures per image), so three
    Case("three-stage", 3, 3, 8, (4, 1, 1, 0), [(4, 1), (6, 2), (10, 2)], 1, rounding_threshold_bits=6, n_bits=5),
    # no block at all: stem, sum pool, output; 17 channels on the stem; 17 x 3 x 3 outputs; parity-split sites
    Case("zero-blocks", 4, 5, 6, (17, 3, 1, 1), [], 2, rounding_threshold_bits=7, n_bits=5),
    # one input channel, 7x7 stem of stride 2 on an odd image (13 -> 7), a strided FIRST block (7 -> 4); global sum pool
    Case("stem7-strided-first", 5, 1, 13, (4, 7, 2, 3), [(6, 2)], 4, rounding_threshold_bits=6, n_bits=5),
    # MaxPool(3, 1, 1): the candidate 4 -> 6 -> 6 on 7 x 7 reshaped to 2 -> 4 -> 5 (fewer input channels, narrower layers)
    Case("pool311", 6, 2, 7, (4, 1, 1, 0), [(4, 1), (5, 2)], 3, pool1=(3, 1, 1), rounding_threshold_bits=6, n_bits=5),
    # MaxPool(3, 2, 1) on 10 x 10 (-> 5), behind a padded 3x3 stem; one block that widens without a stride
    Case("pool321-img10", 7, 3, 10, (4, 3, 1, 1), [(6, 1)], 5, pool1=(3, 2, 1), rounding_threshold_bits=6, n_bits=5),
    # the wide candidate 3 -> 17 -> 33 reshaped: the 18 channels are written by a 1x1 stem and read by a 1x1 shortcut and one 3x3
    # layer, and every 3x3 layer writes 5
    Case("wide-1x1", 8, 3, 5, (18, 1, 1, 0), [(5, 1)], 2, rounding_threshold_bits=6, n_bits=5),
    # rounding_threshold_bits 5, n_bits 4, bit_width 3
    Case("rtb5-n4-bw3", 9, 3, 7, (5, 3, 1, 1), [(5, 1), (6, 2)], 2, bit_width=3, rounding_threshold_bits=5, n_bits=4),
    # approximate rounding: no one-bit steps; compared within the bound of test_approximate_rounding_small_rings (more than half the
    # outputs equal, none more than 4 units off), not bit for bit.  That bound is a statement about a sample, so the case is shaped for a
    # large one: 7 x 3 x 3 = 63 outputs per image, one block.  Under the compiler's own noise model (tests/simulate_ref.py, the numpy twin
    # of `simulate`, 9000 draws of these three images) at most 18 of the 63 differ, never by more than 2; a first shape with two blocks
    # and 7 outputs per image left half of them or fewer equal in 5.7 % of the model's draws -- and did so on the device
    Case("approximate", 10, 3, 12, (5, 3, 2, 1), [(7, 2)], 1, rounding_threshold_bits=6, n_bits=5, rounding_method="approximate"),
    # the zero-block shape on 18 x 18: BATCH images put 3 x 17 x 18 x 18 = 16 524 elements into the stem's parity-split site, more than
    # the 16 384 bootstraps the session's look-up scratch holds, so the site runs as a full chunk and a remainder of 140
    Case("chunked-site", 11, 5, 18, (17, 3, 1, 1), [], 6, rounding_threshold_bits=7, n_bits=5),
]
SCRATCH_CHUNK = 16384     # ciphertexts per launch of a look-up site (csrc/dctfhe.hip: the session's look-up scratch)
NAMES = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=None)
def compiled(name):
    """the case's CompiledCircuit, compiled once per process"""
    from dctfhe import compile as cc
    case = BY_NAME[name]
    return cc.compile_model(case.model(), case.calib(), **case.compile_kw())


def quantise(c, x):
    """float inputs -> (integers [B, C, H, W], phases [B, n_in]) at the circuit's input encoding"""
    from dctfhe import compile as cc
    q = cc.act_quant(np.asarray(x, np.float64), c.in_scale, True, c.in_bits).astype(np.int64)
    return q, (q.astype(np.uint64) << np.uint64(c.e_in)).reshape(q.shape[0], -1)


def decode(c, phases):
    """output phases -> signed integers at the output's exponent, rounded to nearest"""
    return (np.asarray(phases, np.uint64) + (np.uint64(1) << np.uint64(c.e_out - 1))).view(np.int64) >> np.int64(c.e_out)


@functools.lru_cache(maxsize=None)
def interpreter(name, which="fresh"):
    """oracle.circuit_ref.run_clear on the quantised calibration batch or the fresh inputs -> (decoded outputs, overflow flag)"""
    from oracle import circuit_ref
    case, c = BY_NAME[name], compiled(name)
    out, overflow = circuit_ref.run_clear(c.blob, quantise(c, case.calib() if which == "calib" else case.fresh_inputs())[1])
    vals = decode(c, out)
    vals.setflags(write=False)
    return vals, overflow
