"""What tests/test_pool_policy_host.py and tests/test_gpu_pool_policy.py share: the ImageNet setting of the 5-bit RGB trunk, small -- the
stem, its max pool and the first residual block of ResNet-18 3x224^2 (5 bits, rounding_threshold_bits 7) on a 32x32 crop, closed with an
8x8 average pool.  Some 290 000 bootstraps per image (the rounding chains go by the calibrated accumulator widths), 23 040 of them the
pool's pairwise maxima."""
import numpy as np

CROP = slice(96, 128)
CROP_POOL_PAIRS = 23040


def rgb_crops(n, seed):
    from dctfhe import frontend, synthetic
    tf = frontend.rgb_eval_transform(224)
    return np.stack([tf(im) for im in synthetic.synthetic_images(n, seed)]).astype(np.float32)[:, :, CROP, CROP]


def crop_model():
    from dctfhe import models
    return models.trunk_prefix(models.ResNet18QAT(bit_width=5, in_channels=3, img_size=224), n_blocks=1, avgpool_kernel=8)


def crop_module(pool_policy="exact", configuration=None):
    """-> (QuantizedModule, images): calibrated on the first 12 of 14 crops, the last two are for the runs"""
    from dctfhe.quantized_module import compile_brevitas_qat_model
    x = rgb_crops(14, 7)
    qm = compile_brevitas_qat_model(crop_model(), x[:12], n_bits=5, rounding_threshold_bits=7, p_error=0.01, pool_policy=pool_policy,
                                    configuration=configuration)
    return qm, x


def pool_op(compiled):
    from dctfhe import compile as cc
    (i,) = [i for i, o in enumerate(compiled.ops) if o.type == cc.OP_MAXPOOL]
    return i, compiled.ops[i]


def blob_pool_tier(blob, n_tensors, op_index):
    """ip[4] of the pool's record as the blob carries it (dctfhe/compile.py _encode_record)"""
    import struct
    return struct.unpack_from("<i", blob, 32 + 16 * n_tensors + 96 * op_index + 16 + 4 * 4)[0]
