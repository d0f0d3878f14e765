"""The oracle (oracle/vkt_oracle.c, our restatement) against the COMPILED REFERENCE
(oracle/_ref/libvktref.so: the reference's own serial sources built by oracle/ref/Makefile),
bit for bit, on the CPU.  Every GPU test compares a HIP kernel with the oracle; this module is
what says that the oracle computes what the reference computes.

No tolerances: integer codes are equal, Float32 values are equal bit patterns except that NaN
matches NaN (assert_codes_equal).  Two rules keep undefined behaviour of the reference out of
the comparison; both are computed from the inputs, never from the outputs:

  * Float32 sources under Linear: the reference's sampleLinear leaves hi.x unclamped and reads
    one voxel past the buffer for destination voxels with sx == sdx-1, sy >= sdy-2 and
    sz >= sdz-2 (`past_end_mask`).  Exactly those voxels are left out, at most 10 % of a case
    and 2 % of the module's Float32-Linear voxels (asserted); integer sources compare every
    voxel, since all fractions are 0 and every decoded neighbour is finite.
  * Histogram: a voxel whose bin is outside [0, numBins) makes the reference write outside its
    bin array, so no such voxel is ever handed to it (`assert_bins_in_range`, asserted before
    every call).

The module skips without the library; test_library_is_built_where_the_reference_is does not,
so a broken recipe cannot pass as a skip on a machine that has the reference.
"""
import os

import numpy as np
import pytest

import __graft_entry__ as entry
import test_reference_kat as kat
from backends import OracleBackend, ReferenceBackend
from oracle import binding as ob
from oracle import refbinding as rb
from test_gpu_parity import OPS, assert_codes_equal, rand_codes
from test_gpu_resample_fuzz import FMTS as RESAMPLE_FMTS
from test_gpu_resample_fuzz import dims_pair

needs_ref = pytest.mark.skipif(not rb.available(), reason="oracle/_ref/libvktref.so not built (no reference checkout)")

F32 = np.float32
MAPPINGS = [(0.0, 1.0), (-1.0, 3.0), (0.25, 7.5), (3.0, -1.0)]
ALL_FMTS = [1, 2, 3, 4, 5, 6, 7]
MAX_EXCLUDED_PER_CASE = 0.10
MAX_EXCLUDED_PER_MODULE = 0.02


def test_library_is_built_where_the_reference_is():
    """Not skipped: where the reference checkout exists, build() must have produced the library."""
    if os.path.isdir(os.path.join(entry.REFERENCE, "src", "vkt")):
        assert rb.available(), f"{rb.LIB_PATH} is missing although {entry.REFERENCE} exists: oracle/ref/Makefile failed?"
        rb._load()


@needs_ref
def test_reference_library_is_not_interposed_by_libvolkit():
    """libvolkit.so is loaded RTLD_GLOBAL and exports vkt::* functions with the reference's names;
    the reference library must keep calling its own (oracle/ref/libvktref.map keeps them local).
    Bound to libvolkit's, ComputeAggregatesRange refuses the CPU policy with InvalidValue."""
    try:
        import volkit_amd._lib  # noqa: F401
    except Exception:
        pass  # no libvolkit in this process: nothing to clash with, the call below must still work
    codes = np.arange(24, dtype=np.uint8).reshape(2, 3, 4)
    a = rb.aggregates_range(ob.Volume(codes, 4), (0, 0, 0), (4, 3, 2))
    assert (list(a.argmin), list(a.argmax)) == ([0, 0, 0], [3, 2, 1])


@pytest.fixture(scope="module")
def o():
    return OracleBackend()


@pytest.fixture(scope="module")
def r():
    return ReferenceBackend()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_floats_equal(a, b, what):
    """Bit-exact, NaN matches NaN."""
    assert_codes_equal(bits(a), bits(b), 7, what)


def spike(rng, codes, fmt):
    """Integer operands: zeros and top codes sprinkled in, so that saturation, wrap-around and
    division by zero occur (Float32 operands get their specials from rand_codes)."""
    if fmt != 7:
        flat = codes.reshape(-1)
        idx = rng.choice(flat.size, size=max(2, flat.size // 8), replace=False)
        top = np.iinfo(codes.dtype).max
        flat[idx] = rng.choice(np.array([0, 1, top - 1, top], dtype=codes.dtype), size=idx.size)
    return codes


# ---- codec ----------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("mapping", MAPPINGS)
def test_unmap_every_small_code_and_random_wide_codes(mapping):
    rng = np.random.default_rng(11)
    n = 0
    for fmt in ALL_FMTS:
        if ob.BPV[fmt] <= 2:
            codes = np.arange(256 ** ob.BPV[fmt], dtype=np.uint32).astype(ob.CODE_DTYPE[fmt])
        else:
            edge = np.array([0, 1, 2**31 - 1, 2**31, 2**31 + 1, 2**32 - 257, 2**32 - 129, 2**32 - 2, 2**32 - 1,
                             0x7F800000, 0xFF800000, 0x7FC00000, 0x80000000, 0x00000001], dtype=np.uint32)
            codes = np.concatenate([edge, rng.integers(0, 2**32, 4000, dtype=np.uint64).astype(np.uint32)])
        # formats without a codec case leave the value alone: 123 must survive in both
        assert_floats_equal(ob.unmap_array(codes, fmt, *mapping, init=123.0),
                            rb.unmap_array(codes, fmt, *mapping, init=123.0), f"unmap fmt={fmt} {mapping}")
        n += codes.size
    print(f"codec unmap {mapping}: {n} codes")


def map_inputs(rng, fmt, lo, hi):
    span = hi - lo  # negative for the reversed mapping
    vals = [lo + span * rng.uniform(-0.5, 1.5, 3000), lo + span * rng.uniform(0.0, 1.0, 1500)]
    near = []
    for x in (lo, hi, 0.5 * (lo + hi), 0.0):
        x = F32(x)
        near += [x, np.nextafter(x, F32(np.inf)), np.nextafter(x, F32(-np.inf))]
    special = [0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 3e38, -3e38, 1e30, -1e30,
               lo - 5 * span, hi + 5 * span, lo - 70000 * span, hi + 70000 * span]
    vals += [np.array(near, dtype=np.float64), np.array(special, dtype=np.float64)]
    if fmt != 7 and ob.BPV[fmt] <= 2:
        # midpoints between neighbouring codes, and their float neighbours
        n = 256 ** ob.BPV[fmt]
        c = rng.integers(0, n - 1, 600)
        a = ob.unmap_array(c.astype(ob.CODE_DTYPE[fmt]), fmt, lo, hi).astype(np.float64)
        b = ob.unmap_array((c + 1).astype(ob.CODE_DTYPE[fmt]), fmt, lo, hi).astype(np.float64)
        mid = ((a + b) / 2).astype(np.float32)
        vals += [mid, np.nextafter(mid, F32(np.inf)), np.nextafter(mid, F32(-np.inf)), a, b]
    return np.concatenate([np.asarray(v, dtype=np.float32) for v in vals])


@needs_ref
@pytest.mark.parametrize("mapping", MAPPINGS)
@pytest.mark.parametrize("fmt", ALL_FMTS)
def test_map_and_round_trip(fmt, mapping):
    rng = np.random.default_rng(100 + fmt)
    vals = map_inputs(rng, fmt, *mapping)
    init = 0xA5 if ob.BPV[fmt] == 1 else 0xA5A5  # Int8/Int32 are never written: init survives
    c_o, c_r = ob.map_array(vals, fmt, *mapping, init=init), rb.map_array(vals, fmt, *mapping, init=init)
    assert_codes_equal(c_o, c_r, fmt, f"map fmt={fmt} {mapping}")
    v_o, v_r = ob.unmap_array(c_o, fmt, *mapping), rb.unmap_array(c_r, fmt, *mapping)
    assert_floats_equal(v_o, v_r, f"map->unmap fmt={fmt} {mapping}")
    assert_codes_equal(ob.map_array(v_o, fmt, *mapping, init=init), rb.map_array(v_r, fmt, *mapping, init=init), fmt,
                       f"map->unmap->map fmt={fmt} {mapping}")
    print(f"codec map fmt={fmt} {mapping}: {vals.size} values, 3 stages")


@needs_ref
def test_single_voxel_calls_agree_with_the_batched_ones(o, r):
    for fmt in ALL_FMTS:
        for v in (0.0, 0.5, 1.0, -0.25, 1.5):
            assert o.map(v, fmt) == r.map(v, fmt)
        for code in (0, 1, 0x7F, 0x80, 0xFF):
            data = int(code).to_bytes(4, "little")
            assert bits(ob.unmap_voxel(data, fmt, -1.0, 3.0)) == bits(rb.unmap_voxel(data, fmt, -1.0, 3.0))


# ---- Fill -----------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("fmt", ALL_FMTS)
def test_fill_range(o, r, fmt):
    rng = np.random.default_rng(fmt)
    dims = (13, 7, 5)
    init = rand_codes(rng, fmt, dims[::-1])
    n = 0
    for mapping in MAPPINGS:
        for value in (0.0, 0.1, 0.5, 1.0, 1.5, -0.25, 3.0, np.inf, np.nan):
            for first, last in (((0, 0, 0), dims), ((3, 2, 1), (11, 6, 4)), ((5, 5, 3), (6, 6, 4)), ((4, 4, 4), (4, 6, 5))):
                assert_codes_equal(o.fill_range(fmt, mapping, dims, init.copy(), first, last, value),
                                   r.fill_range(fmt, mapping, dims, init.copy(), first, last, value), fmt,
                                   f"fill fmt={fmt} {mapping} v={value} {first}->{last}")
                n += 1
    print(f"fill fmt={fmt}: {n} cases x {init.size} voxels")


# ---- arithmetic -----------------------------------------------------------------------------
ARITH_DIMS = (13, 7, 5)
# whole volume, a sub-box, a non-zero destination offset (the destination index is x + off)
ARITH_BOXES = [((0, 0, 0), ARITH_DIMS, (0, 0, 0)), ((2, 1, 1), (11, 6, 4), (0, 0, 0)), ((1, 1, 0), (9, 5, 3), (3, 2, 1))]


@needs_ref
@pytest.mark.parametrize("fmt", ALL_FMTS)
@pytest.mark.parametrize("op", OPS)
def test_arithmetic(o, r, op, fmt):
    rng = np.random.default_rng(1000 * OPS.index(op) + fmt)
    shape = ARITH_DIMS[::-1]
    n = 0
    for i, m in enumerate(MAPPINGS):
        # one mapping for all three volumes, then three different ones
        for maps in ([m] * 3, [m, MAPPINGS[(i + 1) % 4], MAPPINGS[(i + 2) % 4]]):
            a = spike(rng, rand_codes(rng, fmt, shape), fmt)
            b = spike(rng, rand_codes(rng, fmt, shape), fmt)
            dinit = rand_codes(rng, fmt, shape)
            for first, last, off in ARITH_BOXES:
                out = o.arith(op, [fmt] * 3, maps, a, b, dinit.copy(), first, last, off)
                ref = r.arith(op, [fmt] * 3, maps, a, b, dinit.copy(), first, last, off)
                # the whole destination: the bytes outside the written box are compared too
                assert_codes_equal(out, ref, fmt, f"{op} fmt={fmt} {maps} {first}->{last}+{off}")
                n += 1
    print(f"{op} fmt={fmt}: {n} cases x {a.size} voxels")


@needs_ref
@pytest.mark.parametrize("op", OPS)
def test_arithmetic_mixed_formats(o, r, op):
    rng = np.random.default_rng(77 + OPS.index(op))
    shape = ARITH_DIMS[::-1]
    for _ in range(12):
        fmts = [int(f) for f in rng.choice(ALL_FMTS, 3)]
        maps = [MAPPINGS[int(i)] for i in rng.integers(0, 4, 3)]
        a = spike(rng, rand_codes(rng, fmts[1], shape), fmts[1])
        b = spike(rng, rand_codes(rng, fmts[2], shape), fmts[2])
        dinit = rand_codes(rng, fmts[0], shape)
        first, last, off = ARITH_BOXES[int(rng.integers(0, 3))]
        assert_codes_equal(o.arith(op, fmts, maps, a, b, dinit.copy(), first, last, off),
                           r.arith(op, fmts, maps, a, b, dinit.copy(), first, last, off), fmts[0],
                           f"{op} fmts={fmts} {maps} {first}->{last}+{off}")


# ---- CopyRange ------------------------------------------------------------------------------
# the pairs, mapping pairs and boxes of test_gpu_general.py::test_copy_convert_phases
CONVERT_PAIRS = [(5, 4), (4, 5), (4, 7), (7, 4), (5, 7), (7, 5), (2, 6), (6, 2), (1, 5), (5, 3)]
CONVERT_MAPS = [((0.0, 1.0), (0.0, 1.0)), ((0.0, 1.0), (-1.0, 3.0)), ((0.25, 7.5), (0.0, 1.0))]
COPY_BOXES = [((0, 0, 0), (37, 9, 4), (0, 0, 0)), ((3, 1, 0), (30, 8, 4), (1, 0, 1)),
              ((-2, -1, -1), (39, 10, 5), (0, 0, 0)), ((5, 2, 1), (12, 3, 2), (7, 5, 3))]


@needs_ref
@pytest.mark.parametrize("maps", CONVERT_MAPS)
@pytest.mark.parametrize("sfmt,dfmt", CONVERT_PAIRS + [(f, f) for f in ALL_FMTS])
def test_copy_range(o, r, sfmt, dfmt, maps):
    """Same format and mapping: the bytewise branch; anything else: unmap -> map."""
    rng = np.random.default_rng(13 * sfmt + dfmt)
    src = rand_codes(rng, sfmt, (4, 9, 37))
    dinit = rand_codes(rng, dfmt, (7, 12, 43))
    for first, last, off in COPY_BOXES:
        assert_codes_equal(o.copy_range(dfmt, maps[1], None, dinit.copy(), sfmt, maps[0], src, first, last, off),
                           r.copy_range(dfmt, maps[1], None, dinit.copy(), sfmt, maps[0], src, first, last, off), dfmt,
                           f"copy {sfmt}->{dfmt} {maps} {first}->{last}+{off}")
    print(f"copy {sfmt}->{dfmt} {maps}: {len(COPY_BOXES)} cases x {dinit.size} voxels")


# ---- Resample -------------------------------------------------------------------------------
def src_index(d, s):
    """Destination index -> source index along one axis: f32 divide, f32 multiply, truncate."""
    x = np.arange(d, dtype=np.float32)
    return (x / F32(d) * F32(s)).astype(np.int32)


def past_end_mask(sd, dd):
    """(z, y, x) mask of the destination voxels whose Linear sample reads one voxel past the
    source buffer in the reference: sx == sdx-1 with the clamped y+1 and z+1 on the last row
    and plane.  From the dims alone."""
    sx, sy, sz = (src_index(d, s) for d, s in zip(dd, sd))
    return ((sz >= sd[2] - 2)[:, None, None] & (sy >= sd[1] - 2)[None, :, None] & (sx == sd[0] - 1)[None, None, :])


def small_dims_pair(rng, src_min=1):
    """dims_pair of the GPU fuzz (integer ratios, down-sampling, collapsed axes, any ratio,
    1-voxel axes), redrawn until the volumes are small enough for a CPU test and, for Float32
    Linear sources, until every source axis has at least `src_min` voxels."""
    while True:
        sd, dd = dims_pair(rng)
        if sd != dd and np.prod(sd) <= 40000 and np.prod(dd) <= 40000 and min(sd) >= src_min:
            return sd, dd


class Tally:
    def __init__(self):
        self.cases = self.voxels = self.f32_linear = self.excluded = 0

    def compare(self, o, r, sd, dd, sf, df, smap, dmap, src, fm, what):
        out = o.resample(df, dmap, dd, sf, smap, src, fm)
        ref = r.resample(df, dmap, dd, sf, smap, src, fm)
        self.cases += 1
        self.voxels += out.size
        if sf == 7 and fm == 1 and sd != dd:
            mask = past_end_mask(sd, dd)
            share = mask.mean()
            assert share <= MAX_EXCLUDED_PER_CASE, f"{what}: {share:.3f} of the case excluded"
            self.f32_linear += out.size
            self.excluded += int(mask.sum())
            out, ref = out.copy(), ref.copy()
            out[mask] = ref[mask] = 0
        assert_codes_equal(out, ref, df, what)

    def check_module_cap(self):
        assert self.f32_linear > 0
        assert self.excluded <= MAX_EXCLUDED_PER_MODULE * self.f32_linear, (self.excluded, self.f32_linear)


@needs_ref
def test_resample_random_geometry(o, r):
    """Every pair of the hot-path formats, three random geometries each (six for Float32 sources),
    both filters, unit and non-unit mappings; Float32 sources carry sparse NaN, +-Inf and -0
    (rand_codes)."""
    rng = np.random.default_rng(5000)
    t = Tally()
    for sf in RESAMPLE_FMTS:
        for df in RESAMPLE_FMTS:
            for case in range(6 if sf == 7 else 3):
                sd, dd = small_dims_pair(rng, src_min=4 if sf == 7 else 1)
                smap = [(0.0, 1.0), (-1.0, 3.0), (0.25, 7.5)][int(rng.integers(0, 3))]
                dmap = [(0.0, 1.0), (-1.0, 3.0)][int(rng.integers(0, 2))]
                src = rand_codes(rng, sf, sd[::-1], floats="mixed")
                for fm in (0, 1):
                    t.compare(o, r, sd, dd, sf, df, smap, dmap, src, fm,
                              f"resample {sd}->{dd} {sf}->{df} {smap}->{dmap} fm={fm}")
    t.check_module_cap()
    print(f"resample: {t.cases} cases, {t.voxels} voxels; Float32 Linear: {t.f32_linear} voxels, "
          f"{t.excluded} excluded ({100.0 * t.excluded / t.f32_linear:.3f} %)")


@needs_ref
def test_resample_past_end_rule_on_the_reference_alone(r):
    """The exclusion rule stays inside both caps for the draw itself (Float32 Linear source dims
    >= 4 per axis), whatever the formats and contents."""
    rng = np.random.default_rng(6000)
    total = excluded = 0
    for _ in range(300):
        sd, dd = small_dims_pair(rng, src_min=4)
        mask = past_end_mask(sd, dd)
        assert mask.mean() <= MAX_EXCLUDED_PER_CASE, (sd, dd, mask.mean())
        total += mask.size
        excluded += int(mask.sum())
    assert excluded <= MAX_EXCLUDED_PER_MODULE * total
    print(f"past-the-end rule over 300 draws: {excluded} of {total} voxels ({100.0 * excluded / total:.3f} %)")


@needs_ref
def test_resample_same_dims_branch(o, r):
    rng = np.random.default_rng(5100)
    t = Tally()
    dims = (7, 5, 3)
    for sf in RESAMPLE_FMTS + [1, 3]:
        for df in RESAMPLE_FMTS + [1, 3]:
            src = rand_codes(rng, sf, dims[::-1], floats="mixed")
            for smap, dmap in (((0.0, 1.0), (0.0, 1.0)), ((0.25, 7.5), (-1.0, 3.0))):
                for fm in (0, 1):
                    t.compare(o, r, dims, dims, sf, df, smap, dmap, src, fm, f"same dims {sf}->{df} {smap}->{dmap} fm={fm}")
    print(f"resample same dims: {t.cases} cases, {t.voxels} voxels")


# ---- Transform ------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("fmt", [4, 5, 7])
def test_transform_range_unary(fmt):
    """The unary form only: the reference declares a binary C++ TransformRange but defines none."""
    rng = np.random.default_rng(40 + fmt)
    shape = (3, 4, 5)
    bpv = ob.BPV[fmt]

    seen = set()

    def unary(x, y, z, b, f, lo, hi):
        seen.add((f, lo, hi))
        for i in range(bpv):
            b[i] = (b[i] + x + 3 * y + 5 * z + i) & 0xFF
        b[bpv] = 0xEE  # beyond the voxel: must not reach the volume

    first, last = (1, 0, 1), (5, 3, 3)
    c1 = rand_codes(rng, fmt, shape)
    vo, vr = ob.Volume(c1.copy(), fmt, -1.0, 3.0), ob.Volume(c1.copy(), fmt, -1.0, 3.0)
    ob.transform_range1(vo, first, last, unary)
    rb.transform_range1(vr, first, last, unary)
    assert_codes_equal(vo.codes, vr.codes, fmt, "unary transform")
    assert not np.array_equal(vo.codes, c1)
    assert seen == {(fmt, -1.0, 3.0)}


# ---- Aggregates -----------------------------------------------------------------------------
AGG_FLOAT_FIELDS = ["min", "max", "mean", "stddev", "var", "sum", "prod"]


def assert_aggregates_equal(a, b, what):
    for f in AGG_FLOAT_FIELDS:
        assert_floats_equal([getattr(a, f)], [getattr(b, f)], f"{what}: {f} oracle={getattr(a, f)!r} ref={getattr(b, f)!r}")
    assert list(a.argmin) == list(b.argmin), f"{what}: argmin"
    assert list(a.argmax) == list(b.argmax), f"{what}: argmax"


def agg_both(codes, fmt, mapping, first, last, what):
    a = ob.aggregates_range(ob.Volume(codes, fmt, *mapping), first, last)
    b = rb.aggregates_range(ob.Volume(codes, fmt, *mapping), first, last)
    assert_aggregates_equal(a, b, what)
    return b


@needs_ref
@pytest.mark.parametrize("fmt", [4, 5, 2, 6, 7, 1])
def test_aggregates(fmt):
    rng = np.random.default_rng(300 + fmt)
    dims = (17, 9, 6)
    n = 0
    for mapping in MAPPINGS:
        floats = rng.uniform(-2.0, 2.0, dims[::-1]).astype(np.float32).view(np.uint32)
        codes = floats if fmt == 7 else rand_codes(rng, fmt, dims[::-1])
        agg_both(codes, fmt, mapping, (0, 0, 0), dims, f"agg fmt={fmt} {mapping} whole")
        # sub-ranges: mean and var still divide by the whole volume's voxel count
        for _ in range(5):
            first = tuple(int(rng.integers(0, d - 1)) for d in dims)
            last = tuple(int(rng.integers(f + 1, d + 1)) for f, d in zip(first, dims))
            b = agg_both(codes, fmt, mapping, first, last, f"agg fmt={fmt} {mapping} {first}->{last}")
            n += 1
            assert b.mean == F32(np.float64(b.sum) / codes.size)
        n += 1
    print(f"aggregates fmt={fmt}: {n} cases x up to {codes.size} voxels, 9 fields each")


@needs_ref
def test_aggregates_ties_and_non_finite():
    dims = (6, 5, 4)
    shape = dims[::-1]
    # ties: the first minimum and the first maximum in z, y, x order win
    for fmt, lo_code, hi_code in ((4, 3, 250), (5, 7, 65000)):
        codes = np.full(shape, 100, dtype=ob.CODE_DTYPE[fmt])
        codes[1, 2, 3] = codes[3, 0, 1] = codes[1, 2, 4] = lo_code
        codes[0, 4, 5] = codes[2, 2, 2] = hi_code
        b = agg_both(codes, fmt, (-1.0, 3.0), (0, 0, 0), dims, f"ties fmt={fmt}")
        assert list(b.argmin) == [3, 2, 1] and list(b.argmax) == [5, 4, 0]
        agg_both(np.full(shape, 9, dtype=ob.CODE_DTYPE[fmt]), fmt, (0.0, 1.0), (1, 1, 1), (5, 4, 3), "constant")
    f = np.random.default_rng(5).uniform(-1, 1, shape).astype(np.float32)
    cases = {"all NaN": np.full(shape, np.nan, np.float32)}
    for name, put in (("+Inf", [np.inf]), ("-Inf", [-np.inf]), ("both Inf", [np.inf, -np.inf]), ("NaN first", [np.nan]),
                      ("Inf twice", [np.inf, np.inf]), ("-0", [-0.0, 0.0])):
        g = f.copy()
        g.reshape(-1)[[0, 57][: len(put)]] = put
        cases[name] = g
    g = f.copy()
    g[2, 3, 1] = np.nan  # a NaN in the middle poisons sum/mean/var but not min/max
    cases["NaN inside"] = g
    for name, vals in cases.items():
        agg_both(vals.view(np.uint32), 7, (0.0, 1.0), (0, 0, 0), dims, name)
        agg_both(vals.view(np.uint32), 7, (0.0, 1.0), (0, 1, 0), (6, 4, 3), name + " sub-range")


# ---- Histogram ------------------------------------------------------------------------------
def assert_bins_in_range(vals, lo, hi, num_bins, what):
    """The reference's bin formula in float32 numpy (as test_reduce.py's
    test_oracle_histogram_formula restates it); every voxel's bin must lie in [0, num_bins)."""
    f = (vals.reshape(-1) - F32(lo)) * (F32(num_bins) / (F32(hi) - F32(lo)))
    ok = (f > -1) & (f < num_bins)
    assert ok.all(), f"{what}: {int((~ok).sum())} voxels would be binned outside [0, {num_bins})"
    return np.bincount(np.trunc(f).astype(np.int64), minlength=num_bins)


def histogram_input(rng, fmt, lo, hi, shape):
    """No top code (it decodes to `hi`, bin numBins), floats in [lo, hi)."""
    if fmt == 7:
        u = rng.uniform(0.0, 1.0, shape)
        vals = np.clip((lo + u * (hi - lo)).astype(np.float32), F32(lo), np.nextafter(F32(hi), F32(lo)))
        vals.reshape(-1)[:3] = [lo, np.nextafter(F32(hi), F32(lo)), -0.0 if lo == 0.0 else lo]
        return vals.view(np.uint32)
    dt = ob.CODE_DTYPE[fmt]
    # UInt32: float(code) rounds to 2^32 for the top 128 codes, which all decode to `hi`
    top = 2**32 - 512 if fmt == 6 else int(np.iinfo(dt).max)
    codes = rng.integers(0, top, size=shape, dtype=np.uint64).astype(dt)
    codes.reshape(-1)[:2] = [0, top - 1]
    return codes


@needs_ref
@pytest.mark.parametrize("num_bins", [1, 7, 256, 1000, 65536])
@pytest.mark.parametrize("fmt", [4, 5, 2, 6, 7])
def test_histogram(fmt, num_bins):
    rng = np.random.default_rng(400 + fmt)
    dims = (19, 11, 7)
    n = 0
    for lo, hi in ((0.0, 1.0), (-1.0, 3.0), (0.25, 7.5)):
        codes = histogram_input(rng, fmt, lo, hi, dims[::-1])
        vals = rb.unmap_array(codes, fmt, lo, hi)
        for first, last in (((0, 0, 0), dims), ((2, 1, 3), (17, 10, 6))):
            box = vals[first[2]:last[2], first[1]:last[1], first[0]:last[0]]
            expect = assert_bins_in_range(box, lo, hi, num_bins, f"hist fmt={fmt} bins={num_bins} ({lo},{hi})")
            ref = rb.histogram_range(ob.Volume(codes, fmt, lo, hi), first, last, num_bins)
            out, skipped = ob.histogram_range(ob.Volume(codes, fmt, lo, hi), first, last, num_bins)
            assert skipped == 0
            np.testing.assert_array_equal(out, ref)
            np.testing.assert_array_equal(ref, expect.astype(np.uint64))
            assert int(ref.sum()) == box.size
            n += 1
    print(f"histogram fmt={fmt} bins={num_bins}: {n} cases x up to {codes.size} voxels")


# ---- the typed-in vectors, reproduced by the compiled reference -----------------------------
KAT_TESTS = ([(kat.test_map_kat, k["id"]) for k in kat.KAT if k["op"] == "map"]
             + [(kat.test_safesum_saturated_wraps, None), (kat.test_sumrange_writes_absolute_index, None),
                (kat.test_sum_with_zero_roundtrips_every_code, "codec_roundtrip_all_u8_codes"),
                (kat.test_sum_with_zero_roundtrips_every_code, "codec_roundtrip_all_u16_codes"),
                (kat.test_resample_index_table, "resample_10_to_7"),
                (kat.test_resample_index_table, "resample_4_to_8_duplicates"),
                (kat.test_resample_float_inf_row, None), (kat.test_resample_linear_equals_nearest_integer, None),
                (kat.test_resample_negative_zero, None)])


def test_every_known_answer_vector_is_covered():
    """Each entry of tests/golden/reference_kat.json is reached by one of the wrapped tests."""
    used = {kid for _, kid in KAT_TESTS if kid} | {
        "safesum_u16_saturated_wraps_to_zero", "sumrange_absolute_destination_index",
        "resample_float_inf_linear_vs_nearest", "resample_linear_equals_nearest_for_integer_formats",
        "resample_linear_negative_zero_becomes_positive"}
    assert used == set(kat.BY_ID)


@needs_ref
@pytest.mark.parametrize("fn,kid", KAT_TESTS, ids=[f"{fn.__name__}-{kid}" for fn, kid in KAT_TESTS])
def test_known_answer_vectors_on_the_reference(r, fn, kid):
    """test_reference_kat.py's checks with the compiled reference as the backend: the vectors
    typed in from the survey are what the reference produces."""
    fn(r, kid) if kid else fn(r)


@needs_ref
def test_reference_sampling_is_what_runs(r):
    """The +Inf vector: the reference's Linear and Nearest rows differ exactly as recorded, so
    the driver really runs the reference's sampleLinear and not a nearest lookup."""
    k = kat.BY_ID["resample_float_inf_linear_vs_nearest"]
    sx, sy, sz = k["src_dims"]
    src = kat.codes_of([kat._f(v) for v in k["src"]], 7).reshape(sz, sy, sx)
    rows = {}
    for fm, key in ((1, "expect_linear_row0"), (0, "expect_nearest_row0")):
        rows[fm] = r.resample(7, k["mapping"], k["dst_dims"], 7, k["mapping"], src, fm)[0, 0, :].view(np.float32)
        exp = np.array([kat._f(v) for v in k[key]], dtype=np.float32)
        np.testing.assert_array_equal(np.isnan(rows[fm]), np.isnan(exp))
        np.testing.assert_array_equal(rows[fm][~np.isnan(exp)], exp[~np.isnan(exp)])
    differ = np.isnan(rows[1]) != np.isnan(rows[0])
    exp_differ = np.isnan(np.array([kat._f(v) for v in k["expect_linear_row0"]], dtype=np.float32)) != \
        np.isnan(np.array([kat._f(v) for v in k["expect_nearest_row0"]], dtype=np.float32))
    assert differ.any()
    np.testing.assert_array_equal(differ, exp_differ)
