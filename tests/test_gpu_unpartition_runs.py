"""The final un-partition through LDS-staged digit runs (k_unpart_runs) and pass 0's 2-byte
tile-local permutation, against the C restatement: every reply, and every exported table row.

The cases are the ones at which the staged runs can go wrong: batch sizes at the wave,
workgroup and partition-tile edges and one of more than 1024 tiles (a histogram block then
holds several tiles and a block's last tile takes its counts from the block's total); tiles
that are a single run (digit 0, digit 255, any digit), runs of 16 (digits cycling over 256),
three long runs, digit sets with gaps (empty digits share their run start with the next present
one), run lengths 1, 2, 3, ... (starts at every alignment, runs across 128-byte lines); one-byte
and four-byte replies; outputs at odd offsets; times that escape the narrow record; an engine
without fold records (an intermediate un-partition in front); hot runs; and the re-ranking
engine, which keeps its own kernel."""
import numpy as np
import pytest

from tests import _partition_cases as C

pytestmark = pytest.mark.gpu


def test_engine_forms(engine_lib, gpu):
    """The engines below are the forms the issue names (so each case runs the path it means to)."""
    assert C.rig().lay["narrow"] and C.rig().lay["fold_records"] and C.rig().lay["hot"]
    assert C.rig(127).lay["narrow"] and not C.rig(128).lay["narrow"]
    assert not C.rig(narrow=False).lay["narrow"]
    assert not C.rig(fold_records=False).lay["fold_records"]
    assert C.rig(rerank=True).lay["rerank"]


@pytest.mark.parametrize("d", [0, 255, 77])
def test_one_digit(engine_lib, gpu, d):
    rg = C.rig()
    outs = C.run(rg, C.one_digit(rg, d))
    for n, (g, r) in zip(C.SIZES, outs):   # arrival order decides: the first three, and only they
        m = min(n, 3)
        assert g[:m].tolist() == [1] * m and r[:m].tolist() == [2, 1, 0][:m]
        assert not g[m:].any() and not r[m:].any()


@pytest.mark.parametrize("d", [0, 255])
@pytest.mark.parametrize("limit", [3, 128])
def test_one_bucket(engine_lib, gpu, d, limit):
    """Many keys of one bucket: single-run tiles whose replies differ from position to position
    (at 2^r_bits keys, a 3 * 4096 + 17 batch asks about six times per key; at TokenLimit 3 about
    half of the replies are grants with 2, 1 or 0 left), one-byte and four-byte."""
    rg = C.rig(limit)
    outs = C.run(rg, C.one_bucket(rg, d, 61 + d))
    g, r = outs[-1]
    if limit == 3:   # the run is not one repeated byte
        assert 0.1 < g.mean() < 0.9 and len(np.unique(r[g == 1])) == 3


@pytest.mark.parametrize("mod", [256, 3])
def test_digits_cycling(engine_lib, gpu, mod):
    rg = C.rig()
    C.run(rg, C.cycling(rg, mod))


def test_digit_gaps(engine_lib, gpu):
    rg = C.rig()
    C.run(rg, C.gaps(rg))


def test_run_lengths_1_2_3(engine_lib, gpu):
    rg = C.rig()
    C.run(rg, C.stairs(rg), sizes=C.SIZES + [32896 + 4096])


def test_random(engine_lib, gpu):
    C.run(C.rig(), C.random_keys(7))


def test_buckets_descending(engine_lib, gpu):
    rg = C.rig()
    C.run(rg, C.descending(rg))


@pytest.mark.parametrize("bit", [0, 7, 8])
def test_two_keys_one_bit_apart(engine_lib, gpu, bit):
    rg = C.rig()
    outs = C.run(rg, C.two_keys(rg, bit))
    for n, (g, r) in zip(C.SIZES, outs):
        m = min(n, 6)
        assert g[:m].tolist() == [1] * m and r[:m].tolist() == [2, 2, 1, 1, 0, 0][:m]
        assert not g[m:].any()


@pytest.mark.parametrize("limit,kw", [(127, {}), (128, {}), (3, {"narrow": False})],
                         ids=["one_byte_127", "four_byte_128", "four_byte_not_narrow"])
def test_reply_widths(engine_lib, gpu, limit, kw):
    rg = C.rig(limit, **kw)
    C.run(rg, C.few_keys(11))
    C.run(rg, C.stairs(rg))


def test_without_fold_records(engine_lib, gpu):
    rg = C.rig(fold_records=False)
    C.run(rg, C.few_keys(17))
    C.run(rg, C.cycling(rg, 256))


def test_hot_runs(engine_lib, gpu):
    """One key takes more than 2048 requests of consecutive batches: from the second batch on
    pass 0 ranks its requests by the run's partition key."""
    rg = C.rig()
    C.run(rg, C.hot_and_random(19), sizes=[3 * 4096 + 17] * 4)


@pytest.mark.parametrize("limit", [3, 128])
def test_unaligned_outputs(engine_lib, gpu, limit):
    rg = C.rig(limit)
    C.run(rg, C.few_keys(13), device=gpu)
    C.run(rg, C.stairs(rg), device=gpu)


def test_rerank_keeps_its_kernel(engine_lib, gpu):
    rg = C.rig(rerank=True)
    C.run(rg, C.few_keys(23))


def test_escaped_times(engine_lib, gpu):
    rg = C.rig()
    assert rg.lay["narrow_pass0"]
    C.run(rg, C.few_keys(29), escapes=True)
    C.run(rg, C.stairs(rg), escapes=True)


@pytest.mark.parametrize("case", ["random", "one_digit", "one_bucket_0", "one_bucket_255", "cycling", "four_byte"])
def test_many_tiles_per_histogram_block(engine_lib, gpu, case):
    rg = C.rig(128) if case == "four_byte" else C.rig()
    make = {"random": C.random_keys(31), "four_byte": C.random_keys(37), "one_digit": C.one_digit(rg, 200),
            "one_bucket_0": C.one_bucket(rg, 0, 67), "one_bucket_255": C.one_bucket(rg, 255, 71),
            "cycling": C.cycling(rg, 256)}[case]
    C.run(rg, make, sizes=[C.BIG], device=gpu)
