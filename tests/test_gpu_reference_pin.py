"""The HIP kernels against the COMPILED REFERENCE (oracle/_ref/libvktref.so), directly and bit
for bit: the thin link that does not pass through our own restatement (oracle/vkt_oracle.c).
Each op here also has its oracle tests elsewhere; the shapes are the smallest that still reach
each kernel family.

Only the library is loaded, never a reference checkout (there is none on a GPU machine); the
module skips where the library was not built.  The two rules of test_reference_pin.py apply:
Float32 sources under Linear leave out the destination voxels whose sample reads one voxel
past the source buffer in the reference (`past_end_mask`, from the dims alone, capped), and no
voxel whose histogram bin lies outside [0, numBins) is handed to the reference (asserted).

sum / mean / var of ComputeAggregates take the bounds derived in test_reduce.py's docstring
(the reference accumulates floats serially, the GPU rounds once); everything else is exact.
"""
import numpy as np
import pytest

from backends import GpuBackend, ReferenceBackend
from oracle import binding as ob
from oracle import refbinding as rb
from test_gpu_parity import assert_codes_equal, rand_codes
from test_reduce import EPS, check_float, check_var, gpu_aggregates, gpu_histogram, takes_moments
from test_reference_pin import (MAX_EXCLUDED_PER_CASE, MAX_EXCLUDED_PER_MODULE, assert_bins_in_range, histogram_input,
                                past_end_mask)

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not rb.available(), reason="oracle/_ref/libvktref.so not built (no reference checkout)")]

UNIT = (0.0, 1.0)
F32_LINEAR = {"voxels": 0, "excluded": 0}


@pytest.fixture(scope="module")
def g():
    return GpuBackend()


@pytest.fixture(scope="module")
def r():
    return ReferenceBackend()


# ---- SumRange UInt16 (the metric workload's op) ---------------------------------------------
@pytest.mark.parametrize("first,last", [((0, 0, 0), (256, 24, 10)),     # whole volume: streaming rows
                                        ((3, 1, 2), (253, 23, 9))])     # sub-box: padded rows
def test_sum_range_uint16(g, r, first, last):
    rng = np.random.default_rng(1)
    shape = (10, 24, 256)
    a, b, d = (rand_codes(rng, 5, shape) for _ in range(3))
    args = ("Sum", [5] * 3, [UNIT] * 3, a, b)
    assert_codes_equal(g.arith(*args, d.copy(), first, last, (0, 0, 0)), r.arith(*args, d.copy(), first, last, (0, 0, 0)),
                       5, f"SumRange UInt16 {first}->{last}")


# ---- Resample -------------------------------------------------------------------------------
def resample_case(g, r, sd, dd, sf, df, smap, dmap, src, fm):
    out = g.resample(df, dmap, dd, sf, smap, src, fm)
    ref = r.resample(df, dmap, dd, sf, smap, src, fm)
    if sf == 7 and fm == 1:
        mask = past_end_mask(sd, dd)
        assert mask.mean() <= MAX_EXCLUDED_PER_CASE
        F32_LINEAR["voxels"] += mask.size
        F32_LINEAR["excluded"] += int(mask.sum())
        out[mask] = ref[mask] = 0
    assert_codes_equal(out, ref, df, f"resample {sd}->{dd} {sf}->{df} {smap}->{dmap} fm={fm}")


@pytest.mark.parametrize("sd,dd", [((32, 24, 16), (64, 48, 32)),    # the smoke() shape: the plane kernel
                                   ((37, 23, 11), (64, 40, 19)),    # non-integer ratio
                                   ((64, 40, 24), (48, 30, 20))])   # the LDS gather
def test_resample_uint16(g, r, sd, dd):
    src = rand_codes(np.random.default_rng(sum(sd)), 5, sd[::-1])
    for fm in (1, 0):
        resample_case(g, r, sd, dd, 5, 5, UNIT, UNIT, src, fm)


@pytest.mark.parametrize("sd,dd", [((48, 40, 24), (64, 52, 30)),
                                   ((100, 8, 6), (128, 9, 7))])     # rows that are not 16-byte multiples
def test_resample_uint8(g, r, sd, dd):
    src = rand_codes(np.random.default_rng(sum(sd)), 4, sd[::-1])
    for fm in (1, 0):
        resample_case(g, r, sd, dd, 4, 4, UNIT, UNIT, src, fm)


def test_resample_float32_linear_with_specials(g, r):
    """About 0.4 % NaN / +-Inf / -0 in the source: the chain and its fix-up path against the
    reference's own sampleLinear."""
    rng = np.random.default_rng(7)
    sd, dd = (24, 20, 12), (40, 33, 17)
    vals = rng.uniform(-0.5, 1.5, sd[::-1]).astype(np.float32)
    flat = vals.reshape(-1)
    idx = rng.choice(flat.size, size=flat.size // 250, replace=False)
    flat[idx] = np.resize(np.array([np.nan, np.inf, -np.inf, -0.0], dtype=np.float32), idx.size)
    for dmap in (UNIT, (-1.0, 3.0)):
        resample_case(g, r, sd, dd, 7, 7, UNIT, dmap, vals.view(np.uint32), 1)
    assert F32_LINEAR["excluded"] <= MAX_EXCLUDED_PER_MODULE * F32_LINEAR["voxels"]
    print(f"Float32 Linear: {F32_LINEAR['voxels']} voxels, {F32_LINEAR['excluded']} excluded")


# ---- CopyRange with conversion, FillRange ---------------------------------------------------
def test_copy_range_float32_to_uint16_non_unit_mapping(g, r):
    rng = np.random.default_rng(9)
    shape = (20, 30, 40)
    src = rng.uniform(-1.5, 3.5, shape).astype(np.float32)
    src.reshape(-1)[:6] = [np.nan, np.inf, -np.inf, -0.0, -1.0, 3.0]
    src = src.view(np.uint32)
    dinit = rand_codes(rng, 5, shape)
    for first, last, off in (((3, 2, 1), (37, 28, 19), (0, 0, 0)), ((5, 4, 3), (30, 20, 15), (2, 3, 1))):
        args = (5, (-1.0, 3.0), None)
        tail = (7, UNIT, src, first, last, off)
        assert_codes_equal(g.copy_range(*args, dinit.copy(), *tail), r.copy_range(*args, dinit.copy(), *tail), 5,
                           f"copy Float32->UInt16 {first}->{last}+{off}")


@pytest.mark.parametrize("fmt", [5, 7])
def test_fill_range(g, r, fmt):
    rng = np.random.default_rng(fmt)
    dims = (37, 23, 11)
    init = rand_codes(rng, fmt, dims[::-1])
    for mapping in (UNIT, (-1.0, 3.0)):
        for value in (0.0, 0.1, 1.0, 1.5, -0.25):
            for first, last in (((0, 0, 0), dims), ((3, 2, 1), (30, 20, 9)), ((5, 5, 5), (6, 6, 6))):
                assert_codes_equal(g.fill_range(fmt, mapping, dims, init.copy(), first, last, value),
                                   r.fill_range(fmt, mapping, dims, init.copy(), first, last, value), fmt,
                                   f"fill fmt={fmt} {mapping} v={value} {first}->{last}")


# ---- ComputeAggregates ----------------------------------------------------------------------
@pytest.mark.parametrize("fmt,mapping", [(5, UNIT), (5, (-1.0, 3.0)), (7, UNIT)])
def test_aggregates(fmt, mapping):
    rng = np.random.default_rng(20 + fmt)
    dims = (64, 24, 10)
    if fmt == 7:
        codes = rng.uniform(-1.5, 2.5, dims[::-1]).astype(np.float32).view(np.uint32)
    else:
        codes = rand_codes(rng, fmt, dims[::-1])
    for first, last in (((0, 0, 0), dims), ((3, 3, 2), (61, 20, 9))):
        got = gpu_aggregates(codes, fmt, *mapping, first, last)
        ref = rb.aggregates_range(ob.Volume(codes, fmt, *mapping), first, last)
        what = f"fmt={fmt} {mapping} {first}->{last}"
        assert (got.min, got.max) == (ref.min, ref.max), what
        assert tuple(got.argmin) == tuple(ref.argmin) and tuple(got.argmax) == tuple(ref.argmax), what
        # the per-voxel float terms, through the reference's own codec
        vals = rb.unmap_array(codes, fmt, *mapping)[first[2]:last[2], first[1]:last[1], first[0]:last[0]].reshape(-1)
        n, nall = vals.size, codes.size
        exact_sum = float(np.sum(vals, dtype=np.float64))
        abs_sum = float(np.sum(np.abs(vals), dtype=np.float64))
        check_float("sum", got.sum, ref.sum, exact_sum, abs_sum, n)
        check_float("mean", got.mean, ref.mean, exact_sum / nall, abs_sum / nall, n)
        d = (vals - np.float32(got.mean)).astype(np.float32)
        d2 = (d * d).astype(np.float32)
        terms_sum = float(np.sum(d2, dtype=np.float64))
        var_terms = float(np.float32(np.float64(np.float32(terms_sum)) / nall))
        check_var(got.var, var_terms, takes_moments(fmt, mapping), what)
        ulp = float(np.spacing(np.float32(ref.var)))
        assert abs(got.var - ref.var) <= n * EPS * terms_sum / nall + ulp, f"var: gpu {got.var} vs reference {ref.var} {what}"


# ---- ComputeHistogram -----------------------------------------------------------------------
@pytest.mark.parametrize("fmt,num_bins", [(5, 256), (5, 10240), (7, 1000)])
def test_histogram(fmt, num_bins):
    rng = np.random.default_rng(30 + fmt)
    dims = (256, 33, 17)
    codes = histogram_input(rng, fmt, *UNIT, dims[::-1])
    vals = rb.unmap_array(codes, fmt, *UNIT)
    for first, last in (((0, 0, 0), dims), ((3, 1, 2), (253, 30, 15))):
        box = vals[first[2]:last[2], first[1]:last[1], first[0]:last[0]]
        assert_bins_in_range(box, *UNIT, num_bins, f"hist fmt={fmt} bins={num_bins}")
        ref = rb.histogram_range(ob.Volume(codes, fmt, *UNIT), first, last, num_bins)
        got = gpu_histogram(codes, fmt, *UNIT, first, last, num_bins)
        np.testing.assert_array_equal(got, ref, err_msg=f"fmt={fmt} bins={num_bins} {first}->{last}")
