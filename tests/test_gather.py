"""GPU tests of the gathered and seeded batch CRC (rpc_crc32_device_gather,
rpc_crc32_batch_gather, rpc_crc32_update).

Inputs are the splitmix64 stream (oracle.splitmix_bytes on the host, fill_random on
the device: the same bytes, nothing large is copied).  Expected values: the oracle's
CRC of every segment, folded per body on the CPU with the oracle's combine; the
small cases also against zlib.crc32(concatenation, seed).  Every body is compared,
equality is exact.
"""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
from oracle import oracle  # noqa: E402
from rpc_amd import _lib  # noqa: E402

DEV = "cuda:0"
EINVAL = -22

SEG_COUNTS = [0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 5000]
SEG_LENGTHS = [0, 1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 20000]


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def dev_u64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


def dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV)


def device_buffer(nbytes, seed):
    base = torch.empty((nbytes + 7) // 8 * 8, dtype=torch.uint8, device=DEV)
    rpc_amd.fill_random(base, seed)
    return base


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    assert "gfx950" in rpc_amd.device_info()
    yield
    assert rpc_amd.device_status() == 0


def fold_expected(seg_crc, seg_len, first, seed=None):
    """Per body: c = seed (or 0); for each segment: c = combine(c, crc_s, len_s)."""
    out = np.empty(len(first) - 1, dtype=np.uint32)
    for i in range(len(first) - 1):
        c = 0 if seed is None else int(seed[i])
        for s in range(int(first[i]), int(first[i + 1])):
            c = oracle.combine(c, int(seg_crc[s]), int(seg_len[s]))
        out[i] = c
    return out


def make_case(seed, counts, buf_bytes, extras=False):
    """A deterministic batch: bodies with the given segment counts; every segment
    at a random (unaligned) place of the buffer, so the segments lie in any memory
    order and overlap freely; lengths cycle through SEG_LENGTHS in a shuffled
    order.  extras: one 300 KiB segment, one segment listed in two bodies, and two
    segments that overlap by half."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, dtype=np.int64)
    nseg = int(counts.sum())
    lens = np.asarray(SEG_LENGTHS, dtype=np.uint32)[rng.integers(0, len(SEG_LENGTHS), nseg)]
    # long bodies: mostly short segments, so that the batch stays small
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    for i in np.flatnonzero(counts > 100):
        a, b = int(first[i]), int(first[i + 1])
        small = rng.random(b - a) < 0.9
        lens[a:b] = np.where(small, lens[a:b] % 18, lens[a:b])
    if extras:
        two = np.flatnonzero(counts == 2)
        lens[int(first[two[0]])] = 300 << 10
    offs = (rng.integers(0, buf_bytes - lens.astype(np.int64), nseg)).astype(np.uint64)
    if extras:
        s_a, s_b = int(first[two[1]]), int(first[two[2]])
        lens[s_a], lens[s_b] = 4097, 4097
        offs[s_b] = offs[s_a] = 12345            # one segment, two bodies
        lens[s_a + 1], lens[s_b + 1] = 1024, 1024
        offs[s_a + 1], offs[s_b + 1] = 70001, 70001 + 512  # two overlapping segments
    return offs, lens, first


class Case:
    def __init__(self, seed, counts, buf_bytes, extras=False):
        self.host = oracle.splitmix_bytes(buf_bytes, seed)
        self.offs, self.lens, self.first = make_case(seed, counts, buf_bytes, extras)
        self.n = len(self.first) - 1
        self.seg_crc = oracle.crc32_batch_mt(self.host, self.offs, self.lens)
        self.seeds = np.random.default_rng(seed + 1).integers(0, 1 << 32, self.n, dtype=np.uint64).astype(np.uint32)
        self.seeds[:3] = [0, 0xFFFFFFFF, 0x1234ABCD][:min(3, self.n)]
        self.want_plain = fold_expected(self.seg_crc, self.lens, self.first)
        self.want_seeded = fold_expected(self.seg_crc, self.lens, self.first, self.seeds)
        self.base = device_buffer(buf_bytes, seed)
        self.d_offs, self.d_lens, self.d_first = dev_u64(self.offs), dev_u32(self.lens), dev_u64(self.first)

    def gather(self, **kw):
        return rpc_amd.device_gather(self.base, self.d_offs, self.d_lens, self.d_first, **kw)

    def body(self, i):
        return b"".join(self.host[int(o):int(o) + int(l)].tobytes()
                        for o, l in zip(self.offs[int(self.first[i]):int(self.first[i + 1])],
                                        self.lens[int(self.first[i]):int(self.first[i + 1])]))


@pytest.fixture(scope="module")
def shapes():
    rng = np.random.default_rng(0x6A7)
    counts = np.concatenate([SEG_COUNTS, rng.integers(1, 7, 3000 - len(SEG_COUNTS))])
    counts[20:26] = 2  # (the extras take three two-segment bodies)
    rng.shuffle(counts)
    return Case(0x6A70001, counts, 8 << 20, extras=True)


def test_shapes(shapes):
    """Case 1 of the issue: ~3,000 bodies of 0 .. 5000 segments (the lane fold up to
    32 segments, the narrow and the wide worklist above), every segment length
    class, a 300 KiB segment on the big-body route, unaligned, unordered, shared and
    overlapping segments -- with seeds, without, and in place."""
    c = shapes
    assert set(SEG_COUNTS) <= set(np.diff(c.first.astype(np.int64)).tolist())
    assert set(SEG_LENGTHS) <= set(c.lens.tolist()) and (300 << 10) in c.lens
    for i in range(0, c.n, 97):  # zlib on the concatenation: a second, independent check of the expected values
        assert zlib.crc32(c.body(i), int(c.seeds[i])) == c.want_seeded[i]
        assert zlib.crc32(c.body(i)) == c.want_plain[i]
    got = u32(c.gather())
    assert np.array_equal(got, c.want_plain), np.flatnonzero(got != c.want_plain)[:10]
    got = u32(c.gather(seed=dev_u32(c.seeds)))
    assert np.array_equal(got, c.want_seeded), np.flatnonzero(got != c.want_seeded)[:10]
    inplace = dev_u32(c.seeds)
    assert c.gather(seed=inplace, out=inplace) is inplace
    got = u32(inplace)
    assert np.array_equal(got, c.want_seeded), np.flatnonzero(got != c.want_seeded)[:10]
    got = u32(c.gather(seed=dev_u32(c.seeds), max_seg_len=300 << 10))  # (a bound changes no result)
    assert np.array_equal(got, c.want_seeded)


def test_unchanged_device_batch_after_gather(shapes):
    """Case 7: device_batch over the same segment list, right after a gather call on
    the same stream (workspace reuse), still equals the oracle."""
    c = shapes
    c.gather(seed=dev_u32(c.seeds))
    got = u32(rpc_amd.device_batch(c.base, c.d_offs, c.d_lens))
    assert np.array_equal(got, c.seg_crc), np.flatnonzero(got != c.seg_crc)[:10]


def test_path_thresholds():
    """The segment counts at which the fold changes path (crc32_gather.h): the
    narrow worklist's last size and the wide one's first (kGatherWideMin = 4096),
    and one tile of a wide body +- 1 (kGatherTile = 16384), in one batch with seeds."""
    rng = np.random.default_rng(0x7E5)
    counts = np.array([4095, 3, 4096, 4097, 0, 16383, 16384, 16385, 2 * 16384, 1])
    nseg = int(counts.sum())
    buf_bytes = 1 << 20
    host = oracle.splitmix_bytes(buf_bytes, 0x7E51)
    lens = rng.integers(0, 41, nseg).astype(np.uint32)
    offs = rng.integers(0, buf_bytes - 64, nseg).astype(np.uint64)
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    seeds = rng.integers(0, 1 << 32, len(counts), dtype=np.uint64).astype(np.uint32)
    want = fold_expected(oracle.crc32_batch(host, offs, lens), lens, first, seeds)
    for i in (0, 2, 6):
        body = b"".join(host[int(o):int(o) + int(l)].tobytes() for o, l in zip(offs[int(first[i]):int(first[i + 1])],
                                                                                lens[int(first[i]):int(first[i + 1])]))
        assert zlib.crc32(body, int(seeds[i])) == want[i]
    got = u32(rpc_amd.device_gather(device_buffer(buf_bytes, 0x7E51), dev_u64(offs), dev_u32(lens), dev_u64(first),
                                    seed=dev_u32(seeds)))
    assert np.array_equal(got, want), np.flatnonzero(got != want)


def test_one_long_body():
    """Case 2: one body of 70,000 segments of 0-40 bytes (the wide worklist: five
    tiles anywhere on the chip, then the fold of their values) beside 10 ordinary
    bodies."""
    rng = np.random.default_rng(0x70000)
    counts = np.concatenate([rng.integers(1, 7, 4), [70000], rng.integers(1, 7, 6)])
    nseg = int(counts.sum())
    buf_bytes = 1 << 20
    host = oracle.splitmix_bytes(buf_bytes, 0x70001)
    lens = rng.integers(0, 41, nseg).astype(np.uint32)
    offs = rng.integers(0, buf_bytes - 64, nseg).astype(np.uint64)
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    seeds = rng.integers(0, 1 << 32, len(counts), dtype=np.uint64).astype(np.uint32)
    seg_crc = oracle.crc32_batch(host, offs, lens)
    base = device_buffer(buf_bytes, 0x70001)
    d = (base, dev_u64(offs), dev_u32(lens), dev_u64(first))
    got = u32(rpc_amd.device_gather(*d, seed=dev_u32(seeds)))
    want = fold_expected(seg_crc, lens, first, seeds)
    long_body = b"".join(host[int(o):int(o) + int(l)].tobytes() for o, l in zip(offs[int(first[4]):int(first[5])],
                                                                                 lens[int(first[4]):int(first[5])]))
    assert zlib.crc32(long_body, int(seeds[4])) == want[4]
    assert np.array_equal(got, want), np.flatnonzero(got != want)
    assert np.array_equal(u32(rpc_amd.device_gather(*d)), fold_expected(seg_crc, lens, first))


def dense_case():
    """Case 3: 70,000 back-to-back segments of 64-700 B in bodies of 1-9 segments."""
    rng = np.random.default_rng(0xDE75E)
    lens = rng.integers(64, 701, 70000).astype(np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    counts = []
    while sum(counts) < lens.size:
        counts.append(min(int(rng.integers(1, 10)), lens.size - sum(counts)))
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    seeds = rng.integers(0, 1 << 32, len(counts), dtype=np.uint64).astype(np.uint32)
    return offs, lens, first, seeds, int(offs[-1]) + int(lens[-1])


def dense_run():
    offs, lens, first, seeds, total = dense_case()
    base = device_buffer(total, 0xDE75F)
    return u32(rpc_amd.device_gather(base, dev_u64(offs), dev_u32(lens), dev_u64(first), seed=dev_u32(seeds)))


def test_dense_segment_pass(tmp_path):
    """The segment pass of a back-to-back segment list takes the dense span mode
    (DESIGN.md 4.9); the same call in a child process with RPCCRC_DENSE=0 (the
    switch is read once per process) takes the rows pass.  Both equal the oracle."""
    offs, lens, first, seeds, total = dense_case()
    host = oracle.splitmix_bytes(total, 0xDE75F)
    want = fold_expected(oracle.crc32_batch_mt(host, offs, lens), lens, first, seeds)
    got = dense_run()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "rows.npy")
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import test_gather as t; t.torch.cuda.set_device(0); "
            "np.save(%r, t.dense_run())") % (os.path.join(repo, "tests"), path)
    env = dict(os.environ, RPCCRC_DENSE="0", PYTHONPATH=repo)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=180, env=env, cwd=repo)
    assert p.returncode == 0, p.stderr[-3000:]
    rows = np.load(path)
    assert np.array_equal(rows, want), np.flatnonzero(rows != want)[:10]


def test_body_past_4gib():
    """Case 4: one body = the same 64 MiB segment listed 65 times (4.06 GiB), seeded:
    bit 32 of the shift and the 64-bit length sum."""
    L, k, seed = 64 << 20, 65, 0x1234ABCD
    crc = oracle.crc32(oracle.splitmix_bytes(L, 0x4617))
    want, unseeded = seed, 0
    for _ in range(k):
        want = oracle.combine(want, crc, L)
        unseeded = oracle.combine(unseeded, crc, L)
    assert want == oracle.combine(seed, unseeded, k * L)  # crc32(seed, X) = combine(seed, crc(X), |X|), |X| > 2^32
    base = device_buffer(L, 0x4617)
    got = u32(rpc_amd.device_gather(base, dev_u64(np.zeros(k)), dev_u32(np.full(k, L)), dev_u64([0, k]),
                                    seed=dev_u32([seed])))
    assert got.tolist() == [want]


@pytest.mark.parametrize("pieces", [1, 7, 4096])
def test_running_form_device(pieces):
    """Case 5: a 1 MiB buffer fed piece by piece through successive device_gather
    calls (one segment per body, `out` is the next call's `seed`) gives rpc_crc32 of
    the whole buffer."""
    L = 1 << 20
    host = oracle.splitmix_bytes(L, 0x5EED5)
    base = device_buffer(L, 0x5EED5)
    cuts = np.linspace(0, L, pieces + 1).astype(np.uint64)
    cuts[1:-1] += np.uint64(3) if pieces > 1 else np.uint64(0)  # unaligned, unequal pieces
    d_offs, d_lens = dev_u64(cuts[:-1]), dev_u32(np.diff(cuts))
    d_first = dev_u64([0, 1])
    acc = dev_u32([0])
    bound = int(np.diff(cuts).max()) if pieces > 1 else 0
    for k in range(pieces):
        rpc_amd.device_gather(base, d_offs[k:k + 1], d_lens[k:k + 1], d_first, seed=acc, out=acc, max_seg_len=bound)
    assert u32(acc).tolist() == [oracle.crc32(host)]
    assert zlib.crc32(host.tobytes()) == oracle.crc32(host)


def test_running_form_host():
    """rpc_crc32_update over host pieces equals rpc_crc32 of the whole buffer; NULL
    data gives 0 and an empty piece leaves the CRC unchanged (zlib's crc32)."""
    L = 1 << 20
    host = oracle.splitmix_bytes(L, 0x5EED6)
    whole = rpc_amd.rpc_crc32(host)
    assert whole == oracle.crc32(host)
    for pieces in (1, 7, 4096):
        cuts = np.linspace(0, L, pieces + 1).astype(np.int64)
        cuts[1:-1] += 3 if pieces > 1 else 0
        c = 0
        for a, b in zip(cuts[:-1], cuts[1:]):
            c = rpc_amd.rpc_crc32_update(c, host[a:b])
        assert c == whole, pieces
    assert rpc_amd.rpc_crc32_update(0xDEADBEEF, None) == 0
    assert rpc_amd.rpc_crc32_update(0xDEADBEEF, None, 17) == 0
    assert rpc_amd.rpc_crc32_update(0xDEADBEEF, b"") == 0xDEADBEEF
    assert rpc_amd.rpc_crc32_update(0xDEADBEEF, b"abc", 0) == 0xDEADBEEF
    assert rpc_amd.rpc_crc32_update(0xDEADBEEF, b"abc", 1 << 32) == 0xDEADBEEF  # len mod 2^32 == 0
    assert rpc_amd.rpc_crc32_update(0x1234ABCD, b"123456789") == zlib.crc32(b"123456789", 0x1234ABCD)


def test_host_call_and_arguments():
    """Case 6: crc32_gather (host memory) equals the device result on a 200-body
    batch; n == 0 is a no-op; nseg == 0 gives the seeds; NULL seg_first, NULL out and
    non-zero flags are RPCCRC_EINVAL."""
    rng = np.random.default_rng(0x200)
    c = Case(0x2000001, np.concatenate([[0, 40, 300], rng.integers(0, 7, 197)]), 1 << 20)
    dev_plain, dev_seeded = u32(c.gather()), u32(c.gather(seed=dev_u32(c.seeds)))
    assert np.array_equal(dev_plain, c.want_plain) and np.array_equal(dev_seeded, c.want_seeded)
    assert np.array_equal(rpc_amd.crc32_gather(c.host, c.offs, c.lens, c.first), dev_plain)
    assert np.array_equal(rpc_amd.crc32_gather(c.host, c.offs, c.lens, c.first, seed=c.seeds), dev_seeded)
    for i in range(0, c.n, 13):
        assert zlib.crc32(c.body(i), int(c.seeds[i])) == dev_seeded[i]

    # n == 0: nothing is touched (the pointers are not even looked at)
    assert _lib.rpc_crc32_device_gather(None, None, None, 0, 0, None, 0, None, None, None) == 0
    assert _lib.rpc_crc32_batch_gather(None, None, None, 0, None, 0, None, None, 0) == 0
    poison = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    rpc_amd.device_gather(c.base, c.d_offs, c.d_lens, dev_u64([0]), out=poison)
    assert u32(poison).tolist() == [0x5A5A5A5A] * 4
    assert rpc_amd.crc32_gather(c.host, [], [], [0]).size == 0

    # nseg == 0, n == 5: every body is empty
    seeds = np.array([0, 1, 0xFFFFFFFF, 0x1234ABCD, 7], dtype=np.uint32)
    zeros = dev_u64(np.zeros(6))
    assert u32(rpc_amd.device_gather(None, None, None, zeros, seed=dev_u32(seeds))).tolist() == seeds.tolist()
    assert u32(rpc_amd.device_gather(None, None, None, zeros)).tolist() == [0] * 5
    assert rpc_amd.crc32_gather(None, [], [], np.zeros(6), seed=seeds).tolist() == seeds.tolist()
    assert rpc_amd.crc32_gather(None, [], [], np.zeros(6)).tolist() == [0] * 5

    # arguments
    out = torch.zeros(c.n, dtype=torch.int32, device=DEV)
    args = [c.base.data_ptr(), c.d_offs.data_ptr(), c.d_lens.data_ptr(), c.offs.size, 0, c.d_first.data_ptr(), c.n,
            None, out.data_ptr(), None]
    assert _lib.rpc_crc32_device_gather(*args) == 0
    for k in (5, 8, 0, 1, 2):  # seg_first, out; base, offsets, lengths with nseg > 0
        bad = list(args)
        bad[k] = None
        assert _lib.rpc_crc32_device_gather(*bad) == EINVAL, k
    torch.cuda.synchronize()
    h_out = np.zeros(c.n, dtype=np.uint32)
    h_first = np.ascontiguousarray(c.first)
    hargs = [c.host.ctypes.data, c.offs.ctypes.data, c.lens.ctypes.data, c.offs.size, h_first.ctypes.data, c.n, None,
             h_out.ctypes.data, 0]
    assert _lib.rpc_crc32_batch_gather(*hargs) == 0 and np.array_equal(h_out, dev_plain)
    for k, v in ((4, None), (7, None), (0, None), (8, 1)):  # seg_first, out, base; flags
        bad = list(hargs)
        bad[k] = v
        assert _lib.rpc_crc32_batch_gather(*bad) == EINVAL, k
