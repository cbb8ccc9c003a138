"""CPU emulation of the gather fold (rpc_amd/csrc/crc32_gather.hip)
against zlib.

Body i of rpc_crc32_device_gather is the concatenation of its segments; with each
segment's (crc, len) the kernels fold
    c = seed (or 0);  for s in order:  c = A_{len_s}(c) ^ crc_s
with every shift A_n applied map by map from the nibble tables
NIB[k][i][j] = A_{2^k bytes}(j << 4i).  The pairs (crc, len) form a monoid under
    (c1, l1) . (c2, l2) = (A_{l2}(c1) ^ c2, l1 + l2),    identity (0, 0),
which is what lets one long body be folded as a tree.  Here the same tables and
the same steps are run in Python with a small "wave": gather_lane_kernel's serial
fold, and gather_block_kernel's per-thread runs (fold_run, four segments per load
batch, identity padding), ordered shuffle-down tree over the lanes (tree_step),
the waves through LDS and a second tree, thread 0's carry across tiles, and a wide
body's two levels (gather_tile_kernel's tile values, folded as segments with
64-bit lengths).
"""
import os
import random
import re
import zlib

import pytest

from oracle import oracle

POLY = 0xEDB88320
X0 = 0x80000000
M32 = 0xFFFFFFFF



def kernel_constant(name):
    """The kernels' own value of a constant (crc32_gather.h), so that the emulation
    below runs with the thresholds the device code is built with."""
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rpc_amd", "csrc",
                       "crc32_gather.h")
    m = re.search(r"constexpr uint32_t %s = (\d+);" % name, open(hdr).read())
    assert m, f"{name} not found in {hdr}"
    return int(m.group(1))


LANE_MAX = kernel_constant("kGatherLaneMax")
RUN_MAX = kernel_constant("kGatherRunMax")


def mulmod(a, b):
    m, p = X0, 0
    for _ in range(32):
        if a & m:
            p ^= b
        m >>= 1
        b = (b >> 1) ^ POLY if b & 1 else b >> 1
    return p


def build_nib(maps=64):  # the kernel's image holds all 64 maps: lengths up to 2^64 - 1
    nib, sq = [], X0 >> 8  # x^8: one zero byte; squared: x^(8 * 2^k)
    for _ in range(maps):
        nib.append([[mulmod(sq, j << (4 * i)) for j in range(16)] for i in range(8)])
        sq = mulmod(sq, sq)
    return nib


NIB = build_nib()


def nib_apply(k, v):
    r = 0
    for i in range(8):
        r ^= NIB[k][i][(v >> (4 * i)) & 15]
    return r


def nib_shift(nbytes, v):  # the kernel's nib_shift: one map per set bit of nbytes
    k = 0
    while nbytes:
        if nbytes & 1:
            v = nib_apply(k, v)
        nbytes >>= 1
        k += 1
    return v


def dot(a, b):
    """The monoid: (c1, l1) . (c2, l2)."""
    return nib_shift(b[1], a[0]) ^ b[0], a[1] + b[1]


def fold_run(pairs, r0, r1, acc):
    """fold_run: acc . pairs[r0] . ... . pairs[r1 - 1], in batches of four with the
    segments past r1 entering as the identity."""
    c, l = acc
    s = r0
    while s < r1:
        batch = [pairs[s + q] if s + q < r1 else (0, 0) for q in range(4)]
        for crc, ln in batch:
            c = nib_shift(ln, c) ^ crc
            l += ln
        s += 4
    return c, l


def tree(vals, width):
    """tree_step for m = 1, 2, ... < width over one wave: every lane reads lane
    t + m (its own value past the wave's end, as __shfl_down), and the lanes with
    (t & (2m - 1)) == 0 take it on their right.  Lane 0 ends with the product."""
    vals = list(vals)
    m = 1
    while m < width:
        got = [vals[t + m] if t + m < len(vals) else vals[t] for t in range(len(vals))]
        vals = [dot(vals[t], got[t]) if t & (2 * m - 1) == 0 else vals[t] for t in range(len(vals))]
        m <<= 1
    return vals[0]


def lane_fold(pairs, seed):
    """gather_lane_kernel: a body of <= kGatherLaneMax segments, one lane."""
    assert len(pairs) <= LANE_MAX
    return fold_run(pairs, 0, len(pairs), (seed, 0))[0]


def block_tile(pairs, r0, r1, R, wave, nw):
    """block_tile<NT = wave * nw>: the product of pairs[r0:r1] (at most NT runs of R)
    by one workgroup: runs, lanes, waves."""
    nt = wave * nw
    assert r1 - r0 <= nt * R
    lanes = []
    for t in range(nt):
        a, b = min(r0 + t * R, r1), min(r0 + t * R + R, r1)
        lanes.append(fold_run(pairs, a, b, (0, 0)))
    waves = [tree(lanes[w * wave:(w + 1) * wave], wave) for w in range(nw)]  # wave_c / wave_l
    first = [waves[t] if t < nw else (0, 0) for t in range(wave)]              # wave 0 reads them back
    return tree(first, nw)


def block_fold(pairs, seed, wave, nw, run_max=RUN_MAX):
    """gather_block_kernel (NT = wave * nw): one workgroup per body, tiles of NT
    runs, thread 0 carries them forward from the seed."""
    nt = wave * nw
    p1 = len(pairs)
    per = (p1 + nt - 1) // nt
    R = min(per, run_max) or 1
    carry = seed
    base = 0
    while base < p1:
        c, l = block_tile(pairs, base, min(p1, base + R * nt), R, wave, nw)
        carry = nib_shift(l, carry) ^ c
        base += R * nt
    return carry


def wide_fold(pairs, seed, wave, nw_tile, nw_fold, run_max=RUN_MAX):
    """A wide body: gather_tile_kernel (NT = wave * nw_tile) stores the pair of every
    tile of NT * run_max segments, then gather_block_kernel<1> folds the tile values
    (their lengths are 64-bit sums) as a narrow body's segments."""
    nt = wave * nw_tile
    tile = nt * run_max  # kGatherTile
    tiles = []
    for r0 in range(0, len(pairs), tile):
        r1 = min(len(pairs), r0 + tile)
        tiles.append(block_tile(pairs, r0, r1, (r1 - r0 + nt - 1) // nt, wave, nw_tile))
    return block_fold(tiles, seed, wave, nw_fold, run_max)


def make_segs(rnd, lens):
    segs = [rnd.randbytes(n) for n in lens]
    # the segment pass stores rpc_crc32 of each segment: 0 for an empty one
    return segs, [(zlib.crc32(s), len(s)) for s in segs]


SEEDS = [0, 0xFFFFFFFF, 0x1234ABCD]


def test_nib_shift_is_zlib_combine():
    rnd = random.Random(11)
    for _ in range(30):
        a = rnd.randbytes(rnd.randint(0, 64))
        b = rnd.randbytes(rnd.randint(0, 3000))
        assert nib_shift(len(b), zlib.crc32(a)) ^ zlib.crc32(b) == zlib.crc32(a + b)
        assert nib_shift(len(b), zlib.crc32(a)) ^ zlib.crc32(b) == oracle.combine(zlib.crc32(a), zlib.crc32(b), len(b))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("nseg", [0, 1, 2, 3, 4, 5, 31, 32])
def test_lane_fold_matches_zlib(nseg, seed):
    rnd = random.Random(nseg * 17 + 1)
    segs, pairs = make_segs(rnd, [rnd.choice([0, 1, 15, 16, 17, 300, 1024]) for _ in range(nseg)])
    assert lane_fold(pairs, seed) == zlib.crc32(b"".join(segs), seed)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("wave,nw", [(4, 1), (4, 2), (8, 2), (8, 4)])
def test_block_fold_matches_zlib(wave, nw, seed):
    """NT - 1, NT, NT + 1 segments (one run each, a second tile of one), a tile of
    full runs +- 1, and several tiles with a ragged last one."""
    nt = wave * nw
    rnd = random.Random(wave * 100 + nw)
    for nseg in [1, 2, nt - 1, nt, nt + 1, 2 * nt + 3, nt * RUN_MAX - 1, nt * RUN_MAX, nt * RUN_MAX + 1,
                 3 * nt * RUN_MAX + 5]:
        segs, pairs = make_segs(rnd, [rnd.randint(0, 40) for _ in range(nseg)])
        assert block_fold(pairs, seed, wave, nw) == zlib.crc32(b"".join(segs), seed), nseg


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("wave,nw_tile,nw_fold", [(4, 2, 1), (8, 2, 1)])
def test_wide_fold_matches_zlib(wave, nw_tile, nw_fold, seed):
    """A wide body through the tile pass and the fold of the tile values: one
    tile, a tile +- 1 segment, several tiles, and (run limit 2) more tiles than one
    fold tile holds, so that the second level carries too."""
    rnd = random.Random(wave * 10 + nw_tile)
    tile = wave * nw_tile * RUN_MAX
    for nseg in [tile - 1, tile, tile + 1, 3 * tile + 7]:
        segs, pairs = make_segs(rnd, [rnd.randint(0, 12) for _ in range(nseg)])
        assert wide_fold(pairs, seed, wave, nw_tile, nw_fold) == zlib.crc32(b"".join(segs), seed), nseg
    segs, pairs = make_segs(rnd, [rnd.randint(0, 12) for _ in range(16 * 11 + 3)])  # wave 4: 12 tiles of 16 segments
    assert wide_fold(pairs, seed, wave, nw_tile, nw_fold, run_max=2) == zlib.crc32(b"".join(segs), seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_small_runs_carry_many_tiles(seed):
    """A run limit of 2 makes every body many tiles long: the carry does the work."""
    rnd = random.Random(77)
    for nseg in [9, 16, 17, 40, 41]:
        segs, pairs = make_segs(rnd, [rnd.randint(0, 9) for _ in range(nseg)])
        assert block_fold(pairs, seed, 4, 2, run_max=2) == zlib.crc32(b"".join(segs), seed), nseg


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("where", ["first", "middle", "last", "all"])
def test_empty_segments(where, seed):
    rnd = random.Random(5)
    for nseg in [1, 3, 9, 40]:
        lens = [rnd.randint(1, 50) for _ in range(nseg)]
        for k in {"first": [0], "middle": [nseg // 2], "last": [nseg - 1], "all": range(nseg)}[where]:
            lens[k] = 0
        segs, pairs = make_segs(rnd, lens)
        want = zlib.crc32(b"".join(segs), seed)
        if where == "all":
            assert want == seed  # a body of empty segments yields its seed
        if nseg <= LANE_MAX:
            assert lane_fold(pairs, seed) == want
        assert block_fold(pairs, seed, 4, 2) == want


def test_length_past_4gib_synthetic():
    """A pair whose second length is 2^32 + 5 (no 4 GiB buffer: the CRCs are just
    numbers), checked through the oracle's combine: bit 32 of the shift, and the
    64-bit length sum through the tree."""
    rnd = random.Random(3)
    big = (1 << 32) + 5
    for _ in range(5):
        c1, c2, c3 = (rnd.getrandbits(32) for _ in range(3))
        assert dot((c1, 7), (c2, big)) == (oracle.combine(c1, c2, big), big + 7)
        pairs = [(c1, 7), (c2, big), (c3, 100)]
        want = oracle.combine(oracle.combine(oracle.combine(0x1234ABCD, c1, 7), c2, big), c3, 100)
        assert lane_fold(pairs, 0x1234ABCD) == want
        assert block_fold(pairs, 0x1234ABCD, 4, 2) == want
        # the tree carries the sum 2^32 + 112 in one element: (c1 . c2) . c3 against c1 . (c2 . c3)
        assert dot(dot(pairs[0], pairs[1]), pairs[2]) == dot(pairs[0], dot(pairs[1], pairs[2]))
        assert dot(dot(pairs[0], pairs[1]), pairs[2])[1] == big + 107


def test_monoid_is_associative_with_identity():
    rnd = random.Random(9)
    for _ in range(200):
        a, b, c = ((rnd.getrandbits(32), rnd.choice([0, 1, 5, 1024, rnd.getrandbits(20), rnd.getrandbits(34)]))
                   for _ in range(3))
        assert dot(dot(a, b), c) == dot(a, dot(b, c))
        assert dot(a, (0, 0)) == a and dot((0, 0), a) == a
