"""The case table of the grid-seam tests: one entry per kernel of csrc/dctfhe.hip that runs a grid-stride loop under the capped launch
(`ew_grid()`: at most 16384 blocks of 256 threads; `launch_expand()` caps k_seeded_expand the same way), so one trip of the loop covers
T = 4 194 304 work items and everything beyond comes from the `+= gridDim.x * blockDim.x` step.  tests/test_gpu_grid_seams.py runs the
cases on the device; tests/test_grid_seams_host.py checks, without a GPU, that the table names every capped launch of the source and that
every case meets the rules below.  TEST INFRASTRUCTURE ONLY.

A case lists the shape it runs and, as plain arithmetic on that shape, the work-item count W of each loop it means to cross (the
`total` / `nblk` / `ntail` expression of the kernel) with the size of the row or element group a work item belongs to.  The rules:
  * W > T, and W > 2 T where `trips` says 3;
  * W is no multiple of 256, so the last trip is partial -- except where the kernel's own count is a multiple of 256 by construction at
    the shape the case has to use; the entry then says why in `whole_blocks` and names what is partial instead;
  * T falls strictly inside a group (T mod group != 0): the first item of the second trip is in the middle of a row, not at its start
    -- except where the group size divides T by construction (`on_boundary`, with the reason).
"""
import struct
from types import SimpleNamespace as NS

CAP_BLOCKS, BLOCK = 16384, 256
T = CAP_BLOCKS * BLOCK                                   # work items of one trip: 4 194 304
PACK16_CHUNK = 16384                                     # ciphertexts per k_pack16 launch at most (dev_keyswitch_pack walks LutScratch chunks)


class Loop:
    """one grid-stride loop a case crosses: W work items in groups of `group` (1: the kernel's index is flat, it divides by nothing);
    whole_blocks: why W is a multiple of 256 here; on_boundary: why T falls between two groups here"""

    def __init__(self, kernel, W, group, trips=2, whole_blocks=None, on_boundary=None):
        self.kernel, self.W, self.group, self.trips, self.whole_blocks, self.on_boundary = kernel, int(W), int(group), trips, whole_blocks, on_boundary

    def problems(self):
        """the rules this loop breaks, as text (empty: none)"""
        out = []
        if self.W <= (self.trips - 1) * T:
            out.append(f"{self.kernel}: W = {self.W} does not reach trip {self.trips} (T = {T})")
        if self.W % BLOCK == 0 and not self.whole_blocks:
            out.append(f"{self.kernel}: W = {self.W} is a multiple of {BLOCK}: the last trip is not partial")
        if self.W % BLOCK != 0 and self.whole_blocks:
            out.append(f"{self.kernel}: W = {self.W} is no multiple of {BLOCK}, the exemption no longer applies: {self.whole_blocks}")
        if T % self.group == 0 and not self.on_boundary:
            out.append(f"{self.kernel}: T = {T} falls on a boundary of the groups of {self.group}")
        if T % self.group != 0 and self.on_boundary:
            out.append(f"{self.kernel}: T = {T} lies inside a group of {self.group}, the exemption no longer applies: {self.on_boundary}")
        return out

    def check(self):
        bad = self.problems()
        assert not bad, "; ".join(bad)
        return self.W


class Case:
    """name, the call it goes through, its shape (a namespace) and loops(shape) -> [Loop]"""

    def __init__(self, name, call, shape, loops):
        self.name, self.call, self.shape, self._loops = name, call, NS(**shape), loops

    def loops(self, shape=None):
        return self._loops(self.shape if shape is None else shape)

    def kernels(self):
        return {l.kernel for l in self.loops()}


def _pool_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def _pool_loops(s):
    Ho, Wo = _pool_out(s.H, s.k, s.s, s.p), _pool_out(s.W, s.k, s.s, s.p)
    out = [Loop("k_maxpool_clear", s.C * s.H * Wo, Wo)]                               # the row pass: [B C H][Wo] outputs
    if s.column_pass_crosses:
        out.append(Loop("k_maxpool_clear", s.C * Ho * Wo, Ho * Wo))                    # the column pass: [B C][Ho][Wo] outputs
    return out


SESSION_ROWS = 57 * 4 * 6 * 6            # the levelled session below: batch x C x H x W

CASES = [
    # ---- stand-alone primitives (C ABI, no keys): rows at production strides 513 / 1025 / 2049
    Case("add-2-trips", "dctfhe_add_rows", dict(dim_a=2048, deff_a=1024, dim_b=1024, deff_b=1024, dim_o=2048, rows=2112),
         lambda s: [Loop("k_add", s.rows * (s.dim_o + 1), s.dim_o + 1)]),
    Case("add-3-trips", "dctfhe_add_rows", dict(dim_a=2048, deff_a=1024, dim_b=1024, deff_b=1024, dim_o=2048, rows=4100),
         lambda s: [Loop("k_add", s.rows * (s.dim_o + 1), s.dim_o + 1, trips=3)]),
    Case("affine", "dctfhe_affine_rows", dict(dim_a=1024, deff_a=512, dim_o=2048, nwords=1024, shift=5, rows=4200),
         lambda s: [Loop("k_affine", s.rows * (s.nwords + 1), s.nwords + 1)]),
    Case("acc", "dctfhe_acc_rows", dict(dim_o=2048, dim_b=1024, nwords=1024, rows=4200),
         lambda s: [Loop("k_acc_rows", s.rows * (s.nwords + 1), s.nwords + 1)]),
    Case("gather", "dctfhe_gather_rows", dict(n_src=300, dim_s=1024, deff_s=512, count=2112, dim_d=2048),
         lambda s: [Loop("k_pool_gather", s.count * (s.dim_d + 1), s.dim_d + 1)]),
    Case("sum-pool", "dctfhe_sum_pool_rows", dict(B=1, C=2, H=66, W=66, K=2, dim_in=512, deff_in=512, dim_o=2048),
         lambda s: [Loop("k_sum_pool", s.B * s.C * (s.H // s.K) * (s.W // s.K) * (s.dim_o + 1), s.dim_o + 1)]),
    # the mask loop: one work item per generator block of 8 words, (dim_eff + 7) / 8 + 1 blocks per row
    Case("expand-mask-loop", "dctfhe_expand_seeded", dict(D=1024, dim_eff=1024, dim=1024, rows=32600),
         lambda s: [Loop("k_seeded_expand", s.rows * ((s.dim_eff + 7) // 8 + 1), (s.dim_eff + 7) // 8 + 1)]),
    # the tail loop: the zeros between dim_eff and the body, and the body
    Case("expand-tail-loop", "dctfhe_expand_seeded", dict(D=1024, dim_eff=8, dim=1024, rows=4200),
         lambda s: [Loop("k_seeded_expand", s.rows * (s.dim + 1 - s.dim_eff), s.dim + 1 - s.dim_eff)]),
    # ---- clear mode: one word per element
    # (3 x 1200 x 1200 = 4 320 000 is 16875 whole blocks; one more column makes the last trip partial: 4 323 600)
    Case("lut-clear", "dctfhe_session_run (clear)", dict(C=3, H=1200, W=1201, p=7, r=3, w=4),
         lambda s: [Loop("k_lut_clear", s.C * s.H * s.W, s.H * s.W)]),
    Case("maxpool-clear-2-1-0", "dctfhe_max_pool_rows (keys = NULL)", dict(C=2, H=1500, W=1500, k=2, s=1, p=0, column_pass_crosses=True), _pool_loops),
    Case("maxpool-clear-3-2-1", "dctfhe_max_pool_rows (keys = NULL)", dict(C=8, H=1060, W=1060, k=3, s=2, p=1, column_pass_crosses=False), _pool_loops),
    # ---- a levelled circuit in an encrypted session: y = x + x, then a sum pool of window 1, on 57 images of 4 x 6 x 6 stored at 512 + 1 words
    Case("session-levelled", "dctfhe_session_upload_rows / _run / _download_rows",
         dict(batch=57, C=4, H=6, W=6, deff=512, dim=1024, stride=513),
         lambda s: [Loop("k_tail_nonzero", s.batch * s.C * s.H * s.W * (s.dim - s.deff), s.dim - s.deff,
                         whole_blocks="the upload form is dim = 1024 over a stored 512, so every row has 512 tail words; the guard's seam is "
                                      "tested by the row that holds the non-zero word instead (the last row: items above T)",
                         on_boundary="512 tail words per row divide T; the kernel's x / tail and x % tail are still exercised beyond T"),
                    Loop("k_restride", s.batch * s.C * s.H * s.W * s.stride, s.stride),                       # upload: host rows -> stored rows
                    Loop("k_restride", s.batch * s.C * s.H * s.W * (s.dim + 1), s.dim + 1, trips=3),          # download: stored rows -> host rows
                    Loop("k_add", s.batch * s.C * s.H * s.W * s.stride, s.stride),
                    Loop("k_sum_pool", s.batch * s.C * s.H * s.W * s.stride, s.stride)]),
    # ---- ring pack and public-key draws on the test ring (N = 256)
    Case("ring-digits", "dctfhe_ring_pack", dict(logN=8, n=48, l=1, beta=16, count=87600),
         lambda s: [Loop("k_ring_digits", -(-s.count // (1 << s.logN)) * s.n * (1 << s.logN), s.n * (1 << s.logN),
                         whole_blocks="W = groups n N with N = 256; the last GROUP is partial instead (count mod N != 0: its slots beyond the "
                                      "results are skipped inside the last trip)")]),
    Case("pk-draws", "dctfhe_public_key_draws", dict(logN=8, count=4200000),
         lambda s: [Loop("k_pk_draws", -(-s.count // (1 << s.logN)) * (1 << s.logN), 1 << s.logN,
                         whole_blocks="W = nmask = groups N with N = 256; the e2 draws stop at count, inside the last block, instead",
                         on_boundary="N = 256 divides T; the kernel's index is flat (draw x of three streams), a group is only the e1 cut")]),
]

# kernels whose seam another test already crosses: node ids
COVERED_ELSEWHERE = {
    "k_dct_frontend": "tests/test_gpu_frontend_jpeg.py::test_second_grid_stride_trip",
}
# kernels whose capped launch cannot reach a second trip, with the reason test_grid_seams_host.py checks
CANNOT_CROSS = {
    "k_pack16": "ew_grid(words / 4) over chunks of at most 16384 ciphertexts of n + 1 words: a second trip needs n + 1 > 1024, and every "
                "tier of every shipped catalogue has n <= 1023",
}


def table():
    """kernel -> what covers it: a list of (case, loop), a node id, or the reason it cannot cross"""
    out = {}
    for c in CASES:
        for l in c.loops():
            out.setdefault(l.kernel, []).append((c, l))
    for k, v in list(COVERED_ELSEWHERE.items()) + list(CANNOT_CROSS.items()):
        assert k not in out
        out[k] = v
    return out


def get(name):
    return next(c for c in CASES if c.name == name)


# ------------------------------------------------------------------------------------------ hand-written circuit blobs (csrc/circuit.h)
OP_ADD, OP_SUMPOOL, OP_LUT = 2, 3, 4
LUT_EXACT, LUT_APPROX, LUT_SPLIT = 0, 1, 2


def pack_blob(shapes, records, input_tensor, output_tensor, max_bit_width=7):
    """BlobHeader, the TensorShape table, the Op records, then the payloads (16-byte aligned) the records point at.
    records: dicts of type, src0, src1, dst, ip (12 ints), lp0, payload (bytes)"""
    head = struct.pack("<IIiiiiii", 0x46544344, 1, len(shapes), len(records), input_tensor, output_tensor, max_bit_width, 0)
    tens = b"".join(struct.pack("<iiii", *s, 0) for s in shapes)
    off = len(head) + len(tens) + 96 * len(records)
    recs, payloads = b"", b""
    for r in records:
        assert len(r["ip"]) == 12
        lp0 = r.get("lp0", 0)
        lp0 = lp0 - (1 << 64) if lp0 >= (1 << 63) else lp0
        pay = r.get("payload", b"")
        recs += struct.pack("<iiii12i2qqq", r["type"], r["src0"], r.get("src1", 0), r["dst"], *r["ip"], lp0, 0, off + len(payloads) if pay else 0, len(pay))
        payloads += pay + b"\0" * ((-len(pay)) % 16)
    return head + tens + recs + payloads


def lut_blob(shape, p, r, w, shift, body_add, mode, tables):
    """one OP_LUT on a tensor of `shape` = (C, H, W); tables: int64 [ntab, 2^w] as bytes-convertible numpy (1 table or one per channel)"""
    ntab = tables.shape[0]
    assert tables.shape == (ntab, 1 << w) and str(tables.dtype) == "int64"
    ip = [p, r, w, shift, 0, 1, ntab, -1, 1, mode, 0, -1]      # table tier 0, bit tier 1, no hand-over to a twin, deff_in unused in clear mode
    return pack_blob([shape, shape], [dict(type=OP_LUT, src0=0, dst=1, ip=ip, lp0=int(body_add), payload=tables.tobytes())], 0, 1)


def levelled_blob(shape, deff):
    """tensor 1 = tensor 0 + tensor 0 (OP_ADD, src0 = src1), tensor 2 = sum pool of window 1 of tensor 1; ip[10] = deff: the input is
    stored at that effective dimension"""
    ip_add = [0] * 12
    ip_add[10] = deff
    ip_pool = [1] + [0] * 11
    ip_pool[10] = deff
    return pack_blob([shape] * 3, [dict(type=OP_ADD, src0=0, src1=0, dst=1, ip=ip_add), dict(type=OP_SUMPOOL, src0=1, dst=2, ip=ip_pool)], 0, 2)
