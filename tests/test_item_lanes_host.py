"""How the resident loop's log-domain synchrotron items share their lanes (naima_amd/csrc/nh_syn2.h:
hs_s2_spread, hs_s2_lane_of, hs_s2_chunk_nodes -- pure functions, the same in the kernel and on the
host) without a GPU: a stand-alone program (tests/item_lanes_host.cpp), built host-only under the
address and undefined-behaviour sanitizers, plans the lanes of a slice from its live energies' first
nodes exactly as k_half_step_run does behind barrier 2.

A slice has ONE chunk count Cd from its mean range and nS = ceil(nA Cd / 64) items; every energy
gets floor(64 nS / nA) chunks and the first ones of the compacted order -- the longest ranges when
the photon energies ascend -- one more.  For every set of ranges below:
  * the chunks of all energies fit the planned lanes, and no two lanes hold the same chunk;
  * every piece of every range, from its aligned first node to the grid's end, is covered once;
  * the longest lane is at most one piece above ceil(sum of the pieces / lanes)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

LM, NG, SYN_NODES, CDMAX = 2, 570, 48, 32   # pieces of 4 nodes, the resident loop's 48 nodes per item


@pytest.fixture(scope="module")
def lanes(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("item_lanes") / "item_lanes_host")
    subprocess.run([HIPCC, "--cuda-host-only", "-x", "hip", "-std=c++17", "-O1", "-g",
                    "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "item_lanes_host.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)

    def run(lengths, nG=NG, lm=LM, syn_nodes=SYN_NODES, cdmax=CDMAX):
        """range lengths (nG minus the first live node), in the compacted order -> (plan, lanes)"""
        first = [nG - n for n in lengths]
        Z = [97 + 3 * a for a in range(len(lengths))]   # (every alignment of a range's start to a piece)
        tok = [lm, nG, syn_nodes, cdmax, len(lengths)]
        for i0, z in zip(first, Z):
            tok += [i0, z]
        r = subprocess.run([exe], input=" ".join(str(t) for t in tok), capture_output=True, text=True)
        assert r.returncode == 0 and "runtime error" not in r.stderr and \
            "AddressSanitizer" not in r.stderr, r.stderr  # (clean under both sanitizers)
        out = r.stdout.splitlines()
        plan = {k: int(v) for k, v in (kv.split("=") for kv in out[0].split()[1:])}
        rows = [tuple(int(x) for x in line.split()[1:]) for line in out[1:]]
        return plan, rows, first, Z

    return run


def _check(plan, rows, first, Z, nG=NG, lm=LM, cdmax=CDMAX):
    m = 1 << lm
    nA = len(first)
    assert plan["nA"] == nA
    assert len(rows) == 64 * plan["nS"]
    busy = [r for r in rows if r[1] >= 0]
    # the chunks of all energies fit the planned lanes; a (energy, chunk) pair has one lane
    assert len({(a, ch) for _, a, ch, _, _, _ in busy}) == len(busy) <= 64 * plan["nS"]
    cover = {}
    for _, a, ch, cda, kb, n in busy:
        assert 0 <= a < nA and 0 <= ch < cda <= cdmax
        assert cda == plan["cd"] + (1 if a < plan["nx"] else 0)
        assert kb % m == 0 and (n == 0 or kb + n - 1 <= Z[a] + nG - 1)
        for k in range(kb, kb + n):
            cover[(a, k)] = cover.get((a, k), 0) + 1
    pieces = 0
    longest = 0
    for a in range(nA):
        k0 = ((Z[a] + first[a]) >> lm) << lm
        kend = Z[a] + nG - 1
        # every node from the aligned first one to the grid's last: once
        assert [cover.get((a, k), 0) for k in range(k0, kend + 1)] == [1] * (kend - k0 + 1)
        assert sum(1 for (aa, _) in cover if aa == a) == kend - k0 + 1
        assert sum(1 for r in busy if r[1] == a) == plan["cd"] + (1 if a < plan["nx"] else 0)
        pieces += (kend - k0 + 1 + m - 1) // m
    for _, a, ch, cda, kb, n in busy:
        longest = max(longest, (n + m - 1) // m)
    if nA:
        fair = -(-pieces // (64 * plan["nS"]))
        assert longest <= fair + 1, (longest, fair, plan)
    return longest


def test_all_ranges_equal(lanes):
    plan, rows, first, Z = lanes([200] * 36)
    _check(plan, rows, first, Z)
    assert plan["Cd"] == 5 and plan["nS"] == 3 and plan["cd"] == 5 and plan["nx"] == 12


def test_cfg3_ranges_170_to_234(lanes):
    """the headline's 36 live energies at p0: the longest lane falls from 12 pieces (49 nodes with its
    start node) to 11, and no lane of the three items is idle"""
    lengths = [234 - round(64 * a / 35) for a in range(36)]  # (the lowest energy has the longest range)
    assert lengths[0] == 234 and lengths[-1] == 170
    plan, rows, first, Z = lanes(lengths)
    longest = _check(plan, rows, first, Z)
    assert plan["Cd"] == 5 and plan["nS"] == 3
    assert (plan["cd"], plan["nx"]) == (5, 12)
    assert all(r[1] >= 0 for r in rows)
    assert longest <= 11
    # (one chunk count for all: ceil(ceil(236 / 5) / 4) = 12 pieces)


def test_ranges_in_the_other_order_are_still_covered_once(lanes):
    """descending photon energies: nothing is balanced, everything is covered"""
    lengths = [170 + round(64 * a / 35) for a in range(36)]
    plan, rows, first, Z = lanes(lengths)
    m = 1 << LM
    cover = {}
    for _, a, ch, cda, kb, n in rows:
        if a >= 0:
            for k in range(kb, kb + n):
                cover[(a, k)] = cover.get((a, k), 0) + 1
    for a in range(36):
        k0 = ((Z[a] + first[a]) >> LM) << LM
        assert [cover.get((a, k), 0) for k in range(k0, Z[a] + NG)] == [1] * (Z[a] + NG - k0)
    assert m == 4


def test_one_live_energy(lanes):
    plan, rows, first, Z = lanes([234])
    _check(plan, rows, first, Z)
    assert plan["nS"] == 1 and plan["cd"] == CDMAX and plan["nx"] == 0  # (the partial sums' room binds)


def test_a_range_shorter_than_one_piece(lanes):
    lengths = [234 - round(64 * a / 34) for a in range(35)] + [2]
    plan, rows, first, Z = lanes(lengths)
    _check(plan, rows, first, Z)
    short = [r for r in rows if r[1] == 35]
    assert sum(1 for r in short if r[5] > 0) == 1  # (one lane walks it, its other chunks start past the end)


def test_no_live_energy(lanes):
    plan, rows, first, Z = lanes([])
    assert plan["nS"] == 0 and rows == []


@pytest.mark.parametrize("nA,syn_nodes,cdmax", [(64, 48, 32), (64, 16, 32), (5, 10, 32), (36, 48, 5),
                                                (36, 48, 6), (13, 24, 8)])
def test_other_shapes_fit_and_cover(lanes, nA, syn_nodes, cdmax):
    """64 live energies (a full tile), the short items of several workgroups per walker, a chunk cap
    that binds or leaves one to spare"""
    lengths = [300 - 3 * a for a in range(nA)]
    plan, rows, first, Z = lanes(lengths, syn_nodes=syn_nodes, cdmax=cdmax)
    busy = [r for r in rows if r[1] >= 0]
    assert len({(r[1], r[2]) for r in busy}) == len(busy)
    assert max(r[3] for r in busy) <= cdmax and plan["cd"] >= plan["Cd"]
    cover = {}
    for _, a, ch, cda, kb, n in busy:
        for k in range(kb, kb + n):
            cover[(a, k)] = cover.get((a, k), 0) + 1
    for a in range(nA):
        k0 = ((Z[a] + first[a]) >> LM) << LM
        assert [cover.get((a, k), 0) for k in range(k0, Z[a] + NG)] == [1] * (Z[a] + NG - k0)
