"""The pure half of pvol_radiance_batch's slice walk (csrc/pvol_rays_plan.h) without a GPU: where a candidate slice is
cut back (rays_slice_cut, exported as pvol_radiance_slice_cut), which caller streams a slice holds (rays_slice_streams, exported as
pvol_radiance_slice_streams) and the partition check both radiance entry points and the host batches share (streams_partition, which
the second entry runs first).  The rules are restated here from their wording, not from the C, and the library is held to them."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, abi

RAY, CALLER = abi.RADIANCE_RAY_SCRATCH, abi.RADIANCE_CALLER_SCRATCH
U32 = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def pvol():
    return importlib.import_module("cs348b-pbrt_amd.pvol")


# ------------------------------------------------------------------------------------------ the cut

def need(offset, m):
    """bytes of scratch the first m rays of the candidate take: their expanded rays and themselves"""
    return int(offset[m]) * RAY + m * CALLER


def cut_rule(offset, n, budget):
    """All n rays when they fit or n <= 1; else the largest m in [1, n) that fits, rounded down to a multiple of 64 when it is at
    least 64, and never below 1."""
    if n <= 1 or need(offset, n) <= budget:
        return n
    m = max([k for k in range(1, n) if need(offset, k) <= budget], default=1)
    return m - m % 64 if m >= 64 else m


def scan(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)   # n + 1 offsets


def lib_cut(pvol, offset, n, budget):
    offset = np.ascontiguousarray(offset, np.uint32)
    assert len(offset) == n + 1
    return pvol.lib().pvol_radiance_slice_cut(offset.ctypes.data_as(U32), n, budget)


def check_cut(pvol, sizes, budget):
    n, offset = len(sizes), scan(sizes)
    got = lib_cut(pvol, offset, n, budget)
    assert got == cut_rule(offset, n, budget), (list(sizes), budget)

    def fits(m):   # beyond the candidate nothing fits: the candidate itself did not
        return m <= n and need(offset, m) <= budget
    assert 1 <= got <= n
    assert fits(got) or got == 1                              # the result fits, or it is one ray
    if got < n:
        assert not fits(got + 64 if got >= 64 else got + 1)   # ... and the next step up does not
        assert got % 64 == 0 or got < 64                      # whole runs of 64 where that many fit
    return got


def test_cut_no_ray_spawns(pvol):
    per = RAY + CALLER
    for n in (1, 63, 64, 65, 200):
        sizes = np.ones(n, np.uint32)
        assert check_cut(pvol, sizes, per * n) == n           # exactly at the fit boundary: all of them
        assert check_cut(pvol, sizes, per * n + 1) == n
        below = check_cut(pvol, sizes, per * n - 1)
        assert below == {1: 1, 63: 62, 64: 63, 65: 64, 200: 192}[n]
        for m in (1, 63, 64, 65):                             # the boundary of every shorter run
            if m < n:
                for budget in (per * m - 1, per * m, per * m + 1):
                    check_cut(pvol, sizes, budget)
    assert check_cut(pvol, np.ones(200, np.uint32), per * 127 + per - 1) == 64
    assert check_cut(pvol, np.ones(200, np.uint32), per * 128) == 128


@pytest.mark.parametrize("where", [0, -1, 63, 64])
def test_cut_one_tree(pvol, where):
    """one ray's block is a tree of 31 members, every other ray's a single ray"""
    for n in (65, 130, 200):
        sizes = np.ones(n, np.uint32)
        sizes[where] = 31
        offset = scan(sizes)
        budgets = {need(offset, m) + d for m in (1, 2, 63, 64, 65, n - 1, n) for d in (-1, 0, 1)}
        for budget in sorted(b for b in budgets if b > 0):
            check_cut(pvol, sizes, budget)


def test_cut_every_ray_a_tree(pvol):
    per = 31 * RAY + CALLER
    for n in (1, 63, 64, 65, 200):
        sizes = np.full(n, 31, np.uint32)
        for m in {1, 2, 63, 64, 65, n}:
            if m <= n:
                for budget in (per * m - 1, per * m, per * m + 1):
                    check_cut(pvol, sizes, budget)


def test_cut_first_ray_alone_exceeds_the_budget(pvol):
    for sizes in ([31, 1, 1, 1], [31] * 100, [1] * 70, [31] + [1] * 199):
        assert check_cut(pvol, np.array(sizes, np.uint32), RAY + CALLER - 1) == 1   # one ray always goes
        assert check_cut(pvol, np.array(sizes, np.uint32), 1) == 1
    assert lib_cut(pvol, scan([31]), 1, 1) == 1
    assert lib_cut(pvol, scan([]), 0, 1) == 0


def test_cut_random(pvol):
    rng = np.random.default_rng(20261020)
    for _ in range(500):
        n = int(rng.integers(1, 301))
        sizes = rng.choice(np.array([1, 3, 7, 15, 31], np.uint32), n)
        offset = scan(sizes)
        budget = int(rng.integers(need(offset, 1), need(offset, n) + 1))   # from one ray's need up to the whole
        check_cut(pvol, sizes, budget)


# ------------------------------------------------------------------------------------------ the stream table

def lib_table(pvol, streams, n_rays, r0, r1, s):
    """one slice through the library: (table, s0, continued, next s, maxRays), or the status"""
    streams = np.ascontiguousarray(streams)
    table = np.zeros(max(len(streams), 1), abi.STREAM_DTYPE)
    s_io, out3, most = C.c_uint32(s), (C.c_uint32 * 3)(), C.c_uint32(0)
    rc = pvol.lib().pvol_radiance_slice_streams(streams.ctypes.data, len(streams), n_rays, r0, r1, C.byref(s_io), table.ctypes.data, out3,
                                                C.byref(most))
    if rc != abi.PVOL_OK:
        return rc
    return table[:out3[1]].copy(), out3[0], bool(out3[2]), s_io.value, most.value


def walk(pvol, counts, length):
    """A whole call in slices of `length` rays, every property of the tables asserted.  Returns the slices as (r0, r1, s0, rows)."""
    counts = [int(c) for c in counts]
    streams = abi.make_streams(np.arange(len(counts)) + 7, counts, start_draw=np.arange(len(counts)) * 1000)
    streams["end_draw"] = 99
    n_rays, n_streams = sum(counts), len(counts)
    first = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    pieces = [[] for _ in counts]      # per caller stream: (slice number, rays)
    slices, s, r0, k = [], 0, 0, 0
    while r0 < n_rays:
        r1 = min(r0 + length, n_rays)  # the slices tile [0, nRays) by construction; the tables must follow them
        table, s0, continued, s_next, most = lib_table(pvol, streams, n_rays, r0, r1, s)
        assert most == max(counts + [1])
        assert s0 == s and s <= s_next <= n_streams
        # the table partitions [0, n) in order
        at = 0
        for i, row in enumerate(table):
            who = s0 + i               # s0 + index maps a row back to its caller stream
            assert row["first_ray"] == at and row["seed"] == streams[who]["seed"] and row["start_draw"] == streams[who]["start_draw"]
            assert row["end_draw"] == 0
            lo, hi = max(first[who], r0), min(first[who + 1], r1)
            assert row["n_rays"] == max(hi - lo, 0) and (row["n_rays"] > 0 or counts[who] == 0)
            at += int(row["n_rays"])
            pieces[who].append((k, int(row["n_rays"])))
        assert at == r1 - r0
        # continued exactly when the slice's first stream began in an earlier slice
        assert continued == (len(table) > 0 and first[s0] < r0)
        # a cut stream stays for the next slice; one that ends at the boundary does not
        if len(table) and first[s0 + len(table)] > r1:
            assert s_next == s0 + len(table) - 1
        else:
            assert s_next == s0 + len(table)
        slices.append((r0, r1, s0, len(table)))
        s, r0, k = s_next, r1, k + 1
    assert r0 == n_rays and s == n_streams
    for who, got in enumerate(pieces):
        ks = [k for k, _ in got]
        assert sum(m for _, m in got) == counts[who]
        if counts[who]:
            assert ks == list(range(ks[0], ks[0] + len(ks)))   # consecutive slices
        else:
            assert len(ks) == 1                                # an empty stream appears exactly once
    return slices, pieces


def test_table_three_streams_of_100(pvol):
    slices, pieces = walk(pvol, [100, 100, 100], 64)
    assert [(r0, r1) for r0, r1, _, _ in slices] == [(0, 64), (64, 128), (128, 192), (192, 256), (256, 300)]
    assert [s0 for _, _, s0, _ in slices] == [0, 0, 1, 1, 2]           # the cuts 64, 128, 192, 256 fall inside streams 0, 1, 1, 2
    assert pieces == [[(0, 64), (1, 36)], [(1, 28), (2, 64), (3, 8)], [(3, 56), (4, 44)]]
    walk(pvol, [100, 100, 100], 1)


def test_table_one_stream_of_one(pvol):
    for length in (64, 1):
        slices, pieces = walk(pvol, [1], length)
        assert slices == [(0, 1, 0, 1)] and pieces == [[(0, 1)]]


@pytest.mark.parametrize("length", [64, 1])
def test_table_empty_streams(pvol, length):
    walk(pvol, [0, 100, 50], length)              # at the front
    walk(pvol, [0, 0, 5], length)
    walk(pvol, [70, 0, 70], length)               # between two streams with rays
    walk(pvol, [64, 0, 64], length)               # exactly at a slice boundary
    walk(pvol, [64, 0, 0, 64, 0, 64], length)
    _, pieces = walk(pvol, [100, 28, 0], length)  # at the very end, which is a slice boundary too: the last slice takes it
    assert pieces[2] == [((128 - 1) // length, 0)]
    _, pieces = walk(pvol, [100, 0, 0], length)
    assert pieces[1] == pieces[2] == [((100 - 1) // length, 0)]
    _, pieces = walk(pvol, [64, 0, 64], length)   # an empty stream at an inner boundary opens the slice that follows it
    assert pieces[1] == [(64 // length, 0)]


def test_table_random_partitions(pvol):
    rng = np.random.default_rng(4711)
    for _ in range(200):
        n_streams = int(rng.integers(1, 13))
        counts = rng.integers(0, 80, n_streams) * (rng.random(n_streams) > 0.25)
        while counts.sum() > 400:
            counts = counts // 2
        if counts.sum() == 0:
            counts[int(rng.integers(0, n_streams))] = 1
        for length in (64, 1):
            walk(pvol, counts, length)


# ------------------------------------------------------------------------------------------ the partition

def test_streams_partition(pvol):
    def status(first, counts, n_rays, r1=None):
        st = abi.make_streams(range(len(counts)), counts)
        st["first_ray"] = first
        got = lib_table(pvol, st, n_rays, 0, r1 if r1 is not None else min(n_rays, 64), 0)
        return got if isinstance(got, int) else (abi.PVOL_OK, got[4])
    assert status([0, 10, 30], [10, 20, 5], 35) == (abi.PVOL_OK, 20)    # maxRays: the longest stream
    assert status([0, 10, 30], [10, 20, 50], 80) == (abi.PVOL_OK, 50)
    assert status([0, 0, 0], [0, 0, 1], 1) == (abi.PVOL_OK, 1)
    assert status([0, 11, 31], [10, 20, 5], 36) == abi.PVOL_E_INVALID   # a gap
    assert status([0, 9, 29], [10, 20, 5], 34) == abi.PVOL_E_INVALID    # an overlap
    assert status([5, 15, 35], [10, 20, 5], 40) == abi.PVOL_E_INVALID   # does not begin at ray 0
    assert status([10, 0, 30], [20, 10, 5], 35) == abi.PVOL_E_INVALID   # out of order
    assert status([0, 10, 30], [10, 20, 5], 36) == abi.PVOL_E_INVALID   # a short total
    assert status([0, 10, 30], [10, 20, 5], 34) == abi.PVOL_E_INVALID   # a long total
    # the entry's own arguments
    assert status([0, 10, 30], [10, 20, 5], 35, r1=36) == abi.PVOL_E_INVALID
    assert status([0, 10, 30], [10, 20, 5], 35, r1=0) == abi.PVOL_E_INVALID


def test_symbols_are_test_entries(pvol):
    out = subprocess.run(["nm", "-D", "--defined-only", pvol.LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    header = open(os.path.join(ROOT, "include", "pvol.h")).read()
    for sym in ("pvol_radiance_slice_cut", "pvol_radiance_slice_streams"):   # test entries like pvol_plan_batch, not ABI
        assert sym in names and sym not in header and sym not in pvol.EXPORTS, sym
    assert pvol.lib().pvol_abi_version() == 3
    plan = open(os.path.join(ROOT, "cs348b-pbrt_amd", "csrc", "pvol_rays_plan.h")).read()
    includes = [ln.split()[1] for ln in plan.splitlines() if ln.startswith("#include")]
    assert includes and not [i for i in includes if "hip" in i or "pvol_host" in i or "_dev" in i]   # the pure half includes no HIP header
