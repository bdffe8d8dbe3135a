"""The grid-seam case table against the source, without a GPU (tests/grid_seam_cases.py; the device half is tests/test_gpu_grid_seams.py).
Every kernel that csrc/dctfhe.hip launches under the capped grid -- `ew_grid(`, and k_seeded_expand through launch_expand -- must be a key
of the table: a capped launch cannot be added without a case that runs it past its first trip.  The cap and the block size the table
stands on are read from the source too, every case's work counts are recomputed from its shape and held to the rules, and the one kernel
that cannot cross (k_pack16) is held to the reason it cannot."""
import os
import re

import pytest

import grid_seam_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "dct-cryptonets_amd", "csrc", "dctfhe.hip")


@pytest.fixture(scope="module")
def source():
    with open(SRC) as f:
        return f.read()


def capped_kernels(text):
    """every kernel launched with ew_grid(, plus k_seeded_expand (launch_expand computes the same cap itself)"""
    names = set(re.findall(r"hipLaunchKernelGGL\(\s*(\w+)\s*,\s*dim3\(ew_grid\(", text))
    if re.search(r"hipLaunchKernelGGL\(\s*k_seeded_expand\s*,", text):
        names.add("k_seeded_expand")
    return names


def uncovered(kernels, table):
    return sorted(k for k in kernels if k not in table)


def test_cap_and_block_size_are_what_the_table_assumes(source):
    m = re.search(r"static unsigned ew_grid\(size_t n\)\s*\{([^}]*)\}", source)
    assert m, "ew_grid() is gone: the grid-seam table (tests/grid_seam_cases.py) stands on it"
    assert re.search(r"\(n \+ 255\) / 256,\s*16384\)", m.group(1)), f"ew_grid() no longer caps at 16384 blocks of 256: {m.group(1).strip()}"
    assert (G.CAP_BLOCKS, G.BLOCK, G.T) == (16384, 256, 4194304)
    # every capped launch runs blocks of 256 threads
    launches = re.findall(r"hipLaunchKernelGGL\(\s*\w+\s*,\s*dim3\(ew_grid\((?:[^()]|\((?:[^()]|\([^()]*\))*\))*\)\)\s*,\s*dim3\((\d+)\)", source)
    assert len(launches) == len(re.findall(r"dim3\(ew_grid\(", source)) and set(launches) == {"256"}, launches
    # launch_expand: the same cap, written out
    body = source[source.index("static int launch_expand("):]
    body = body[:body.index("\n}\n")]
    assert re.search(r"\(work \+ 255\) / 256,\s*16384\)", body), "launch_expand no longer caps at 16384 blocks of 256"
    assert re.search(r"hipLaunchKernelGGL\(k_seeded_expand, dim3\(grid\), dim3\(256\)", body)
    assert source.count("hipLaunchKernelGGL(k_seeded_expand") == 1, "k_seeded_expand is launched outside launch_expand: is that launch capped?"


def test_table_lists_every_capped_launch(source):
    kernels = capped_kernels(source)
    assert len(kernels) >= 14 and "k_seeded_expand" in kernels and "k_add" in kernels, kernels
    table = G.table()
    missing = uncovered(kernels, table)
    assert not missing, (f"{missing} run a grid-stride loop under the capped launch and have no entry in tests/grid_seam_cases.py: add a case "
                         f"that takes each past T = {G.T} work items (tests/test_gpu_grid_seams.py), or name the test that already does")
    stale = sorted(k for k in table if k not in kernels)
    assert not stale, f"{stale} are in the table and are no longer launched under the cap"


def test_a_kernel_removed_from_the_table_is_noticed(source):
    kernels, table = capped_kernels(source), G.table()
    for k in table:
        assert uncovered(kernels, {x: v for x, v in table.items() if x != k}) == [k]


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.name)
def test_case_shapes_meet_the_rules(case):
    loops = case.loops()
    assert loops
    for l in loops:
        assert l.problems() == [], case.name
        assert l.W < 4 * G.T, "a case stays near the seams it is about: the host reference and the copies are its cost"


def test_rules_bite():
    """the checker itself: each rule refuses what it should"""
    assert G.Loop("k", G.T + 1, 2049).problems() == []
    assert any("does not reach" in p for p in G.Loop("k", G.T, 2049).problems())
    assert any("does not reach trip 3" in p for p in G.Loop("k", 2 * G.T, 2049, trips=3).problems())
    assert any("multiple of 256" in p for p in G.Loop("k", G.T + 256, 2049).problems())
    assert any("boundary" in p for p in G.Loop("k", G.T + 1, 2048).problems())
    assert G.Loop("k", G.T + 256, 2049, whole_blocks="by construction").problems() == []
    assert any("no longer applies" in p for p in G.Loop("k", G.T + 1, 2049, whole_blocks="by construction").problems())
    assert G.Loop("k", G.T + 1, 2048, on_boundary="by construction").problems() == []
    assert any("no longer applies" in p for p in G.Loop("k", G.T + 1, 2049, on_boundary="by construction").problems())


def test_work_counts_are_the_ones_the_shapes_were_chosen_for():
    W = {c.name: [l.W for l in c.loops()] for c in G.CASES}
    assert W["add-2-trips"] == [4327488] and W["add-3-trips"] == [8400900]
    assert W["affine"] == [4305000] and W["acc"] == [4305000] and W["gather"] == [4327488] and W["sum-pool"] == [4462722]
    assert W["expand-mask-loop"] == [4205400] and W["expand-tail-loop"] == [4271400]
    assert W["lut-clear"] == [4323600]
    assert W["maxpool-clear-2-1-0"] == [4497000, 4494002] and W["maxpool-clear-3-2-1"] == [4494400]
    assert W["session-levelled"] == [4202496, 4210704, 8413200, 4210704, 4210704] and G.SESSION_ROWS == 8208
    assert W["ring-digits"] == [343 * 48 * 256] and W["pk-draws"] == [4200192]
    # the look-up case: T lies inside channel 2, so the per-channel table pick (g / hw) % nchan is exercised beyond the seam
    s = G.get("lut-clear").shape
    assert G.T // (s.H * s.W) == 2
    # the three-trip cases
    assert {c.name for c in G.CASES for l in c.loops() if l.trips == 3} == {"add-3-trips", "session-levelled"}


def test_ring_case_is_one_launch():
    """dev_ring_pack batches groups by a 64 MB budget of transposed digits (and at most 4096): the case's groups must fit one launch, or
    its k_ring_digits launches would each stay under T"""
    s = G.get("ring-digits").shape
    N = 1 << s.logN
    groups = -(-s.count // N)
    per_launch = max(1, min(groups, 4096, (64 << 20) // (s.n * s.l * N * 4)))
    assert per_launch == groups == 343 and s.count % N != 0


def test_entries_that_point_elsewhere_point_at_a_test():
    for kernel, node in G.COVERED_ELSEWHERE.items():
        path, name = node.split("::")
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        assert re.search(rf"^def {name}\(", text, re.M), f"{kernel}: {node} does not exist"
        assert "pytest.mark.gpu" in text


def test_pack16_cannot_cross(source):
    """k_pack16's launch is ew_grid(words / 4) with words = chunk (n + 1), chunk <= 16384: a second trip needs n + 1 > 1024"""
    from dctfhe import params as P
    assert "k_pack16" in G.CANNOT_CROSS
    assert re.search(r"hipLaunchKernelGGL\(k_pack16, dim3\(ew_grid\(words / 4\)\)", source), "k_pack16's launch changed: does it cross T now?  Give it a case"
    # the chunk of both callers of dev_keyswitch_pack: the primitive's scratch and a session's
    assert "alloc_lut_scratch(K, std::min<size_t>(count, 16384), &sc)" in source and "sp.scratch_chunk = std::min<size_t>(maxe, 16384)" in source, \
        "the look-up scratch chunk is no longer capped at 16384 ciphertexts: k_pack16 may cross T now, give it a case in tests/grid_seam_cases.py"
    catalogues = {"default_params": P.default_params(), "default_params_5bit": P.default_params_5bit(), "default_params_5bit_pool": P.default_params_5bit_pool(),
                  "params_for_p_error": P.params_for_p_error(), "test_params": P.test_params()}
    shipped = {n for n in dir(P) if re.fullmatch(r"(default_params\w*|params_for_p_error|test_params)", n)}
    assert shipped == set(catalogues), f"a catalogue joined or left dctfhe/params.py: {sorted(shipped ^ set(catalogues))}"
    for name, ps in catalogues.items():
        for t in ps.tiers:
            assert G.PACK16_CHUNK * (t.n + 1) // 4 <= G.T and t.n <= 1023, \
                (f"{name} tier {t.name}: n = {t.n} > 1023, so k_pack16's launch of 16384 rows of n + 1 words now runs a second grid-stride trip: "
                 f"move k_pack16 from CANNOT_CROSS to a case in tests/grid_seam_cases.py")


def test_hand_written_blobs_validate_and_parse():
    """the blobs of the device half: the library's validator accepts them and the oracle's parser reads the same bytes"""
    import ctypes as C

    import numpy as np

    from dctfhe import _lib
    from oracle import circuit_ref
    L = _lib.load()
    L.dctfhe_last_error.restype = C.c_char_p
    s = G.get("lut-clear").shape
    tables = np.arange(3 * 16, dtype=np.int64).reshape(3, 16) * 2
    for mode in (G.LUT_EXACT, G.LUT_APPROX, G.LUT_SPLIT):
        blob = G.lut_blob((s.C, s.H, s.W), s.p, s.r, s.w, 3, 12345, mode, tables)
        assert L.dctfhe_circuit_validate(blob, C.c_size_t(len(blob))) == 0, L.dctfhe_last_error().decode()
        c = circuit_ref.parse_blob(blob)
        assert c["tensors"] == [(3, 1200, 1201)] * 2 and (c["input"], c["output"]) == (0, 1) and len(c["ops"]) == 1
        o = c["ops"][0]
        assert (o["type"], o["src0"], o["dst"], o["ip"][:4], o["ip"][6], o["ip"][9], o["lp"][0]) == (4, 0, 1, (7, 3, 4, 3), 3, mode, 12345)
        assert o["payload"] == tables.tobytes()
    odd = tables.copy()
    odd[1, 4] += 1
    blob = G.lut_blob((s.C, s.H, s.W), s.p, s.r, s.w, 3, 0, G.LUT_SPLIT, odd)
    assert L.dctfhe_circuit_validate(blob, C.c_size_t(len(blob))) != 0 and "odd sum" in L.dctfhe_last_error().decode()
    v = G.get("session-levelled").shape
    blob = G.levelled_blob((v.C, v.H, v.W), v.deff)
    assert L.dctfhe_circuit_validate(blob, C.c_size_t(len(blob))) == 0, L.dctfhe_last_error().decode()
    c = circuit_ref.parse_blob(blob)
    assert c["tensors"] == [(4, 6, 6)] * 3 and (c["input"], c["output"]) == (0, 2)
    assert [(o["type"], o["src0"], o["src1"], o["dst"], o["ip"][0], o["ip"][10]) for o in c["ops"]] == [(2, 0, 0, 1, 0, 512), (3, 1, 0, 2, 1, 512)]
    x = np.arange(2 * 144, dtype=np.uint64).reshape(2, 144) * np.uint64(0x9E3779B97F4A7C15)
    out, ov = circuit_ref.run_clear(blob, x)
    assert not ov and np.array_equal(out, x + x)


def test_vectorised_max_pool_reference_is_the_window_definition():
    """oracle/circuit_ref.max_pool_words takes the maximum tap by tap over strided views (the seam shapes have millions of windows);
    here against the definition written out window by window, padding taps at both borders, signed words, the most negative word too"""
    import numpy as np

    from oracle import circuit_ref
    rng = np.random.default_rng(5)
    for (H, W, k, s, p) in [(7, 9, 2, 1, 0), (9, 7, 3, 2, 1), (6, 6, 2, 2, 1), (5, 8, 3, 1, 1), (8, 8, 4, 3, 2), (3, 3, 3, 1, 1)]:
        x = rng.integers(0, 2 ** 64, (2, 3, H, W), dtype=np.uint64)
        x[0, 0, 0, 0] = x[1, 2, H - 1, W - 1] = np.uint64(1 << 63)           # INT64_MIN: below every padding tap's stand-in, never above a real tap
        xs = x.view(np.int64)
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        want = np.empty((2, 3, Ho, Wo), np.int64)
        for yo in range(Ho):
            ys = [y for y in range(yo * s - p, yo * s - p + k) if 0 <= y < H]
            for xo in range(Wo):
                cols = [c for c in range(xo * s - p, xo * s - p + k) if 0 <= c < W]
                want[:, :, yo, xo] = xs[:, :, ys][:, :, :, cols].max(axis=(2, 3))
        assert np.array_equal(circuit_ref.max_pool_words(x, k, s, p), want.view(np.uint64)), (H, W, k, s, p)
