"""GPU parity: the HIP path (through librpccrc's C-ABI) against the CPU oracle and the
reference golden vectors.  Bit-exact everywhere (integer/byte work).

Small sizes are compared body by body against the oracle; BASELINE.json's full
sizes are checked with size-independent properties (sampled oracle parity,
linearity crc(X)^crc(Y)^crc(X^Y) == crc(0^L), and a checksum of checksums:
the whole buffer as ONE body through the chunked path equals the zlib
crc32_combine fold of the per-body CRCs).
"""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import rpc_amd  # noqa: E402
from oracle import oracle  # noqa: E402

DEV = "cuda:0"


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def to_dev(a: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    info = rpc_amd.device_info()
    assert "gfx950" in info, info
    yield


# ---- drop-in rpc_crc32 / rpc_crc32_verify (crc.c:4-14) ----------------------

def test_drop_in_kats(golden):
    for k in golden["kats"]:
        b = bytes.fromhex(k["hex"])
        assert rpc_amd.rpc_crc32(b) == k["crc"], k["name"]
        assert rpc_amd.rpc_crc32_verify(b, k["crc"])
        assert not rpc_amd.rpc_crc32_verify(b, k["crc"] ^ 1)


def test_drop_in_edges(golden):
    assert rpc_amd.rpc_crc32(None, 5) == 0
    assert rpc_amd.rpc_crc32(b"abc", 0) == 0
    # zlib uInt length: 2**32 + 3 reads exactly 3 bytes
    assert rpc_amd.rpc_crc32(bytes(3), 2**32 + 3) == golden["edges"]["zeros3"]


def test_drop_in_golden_random(golden):
    for r in golden["random_bodies"]:
        data = oracle.splitmix_bytes(r["len"], r["seed"])
        assert rpc_amd.rpc_crc32(data) == r["crc"], r


def test_drop_in_large_bodies():
    # device copy and chunked paths; exact multiples of 16 MiB take the one-row-chunk
    # contiguous combine, whose atomics now target a device word, not
    # the pinned host result; 256 MiB: 64Ki one-row chunks, the rows pass's round values
    for n in [(8 << 20) - 1, (8 << 20) + 13, (17 << 20) + 5, 16 << 20, 32 << 20, 48 << 20, 256 << 20]:
        data = oracle.splitmix_bytes(n, n)
        assert rpc_amd.rpc_crc32(data) == oracle.crc32(data), n


def test_drop_in_staging_pool_with_concurrent_batch():
    """the drop-in path stages bodies > 64 KiB in the device workspace
    pool (stream-ordered, no hipMalloc / hipFree device sync).  > 64 MiB drop-in calls
    on one thread while another thread runs device batches on its own stream; every
    CRC checked, twice (the second round reuses the pooled blocks)."""
    big = [(64 << 20) + 17, (96 << 20), (65 << 20) + 3]
    datas = [oracle.splitmix_bytes(n, 0xB16 + n) for n in big]
    wants = [oracle.crc32(d) for d in datas]
    n, L = 4096, 3000
    host = oracle.splitmix_bytes(n * L, 0xBA7C4)
    base = to_dev(host)
    want_b = oracle.crc32_uniform(host, n, L)
    errors = []
    stop = threading.Event()

    def batches():
        s = torch.cuda.Stream()
        k = 0
        while not stop.is_set() or k < 4:
            with torch.cuda.stream(s):
                got = u32(rpc_amd.device_uniform(base, n, L, stream=s))
            if not np.array_equal(got, want_b):
                errors.append(("batch", k))
            k += 1

    th = threading.Thread(target=batches)
    th.start()
    try:
        for _ in range(2):
            for d, w in zip(datas, wants):
                if rpc_amd.rpc_crc32(d) != w:
                    errors.append(("drop-in", len(d)))
    finally:
        stop.set()
        th.join()
    assert not errors, errors
    assert rpc_amd.device_status() == 0


def test_error_words_per_call_and_clearable():
    """VERDICT r03 #8 / ADVICE r03: a wave that gives up a bounded wait of the
    tail-stealing protocol stores into the error word of ITS call, and the host
    reports RPCCRC_EIO instead of returning stale CRCs with rc 0.
      * synchronous calls (host batch, drop-in) own a word per call: the failing
        call returns -5, the device word stays clear, the next call works;
      * asynchronous calls report through the device word: -5 from
        rpc_crc32_device_status and from every later asynchronous call, until
        rpc_crc32_device_clear_status; synchronous calls keep working meanwhile.
    Forced in a child process on the fault-injection build librpccrc_test.so
    (RPCCRC_TEST_STEAL_GIVEUP=2: the next two stealing launches give up).  (Round 4's
    first version sent one 512 MiB body, whose 16 KiB chunks do not steal: the hook
    then hit the clean call instead.)"""
    import os
    import subprocess
    import sys
    code = r"""
import numpy as np, torch, rpc_amd
from oracle import oracle
torch.cuda.set_device(0)
assert rpc_amd.device_status() == 0
# (a) host batch of 256 x 1 MiB bodies: one stage, every body on the big-body
# route, whose chunk pass deals its tail from a steal pool -> give-up #1
big = oracle.splitmix_bytes(256 << 20, 0xB16E)
offs = np.arange(256, dtype=np.uint64) * np.uint64(1 << 20)
lens = np.full(256, 1 << 20, dtype=np.uint32)
want_big = oracle.crc32_batch(big, offs, lens)
try:
    rpc_amd.crc32_batch(big, offs, lens)
    print("host1", 0)
except rpc_amd.RpcCrcError as e:
    print("host1", e.code)
print("status_after_host", rpc_amd.device_status())
# (b) asynchronous device batch -> give-up #2, recorded in the device word
n, L = 65536, 4096
base = torch.empty(n * L, dtype=torch.uint8, device="cuda:0")
rpc_amd.fill_random(base, 0x6E7)
rpc_amd.device_uniform(base, n, L)
torch.cuda.synchronize()
print("status", rpc_amd.device_status())
try:
    rpc_amd.device_uniform(base, 16, L)
    print("next", 0)
except rpc_amd.RpcCrcError as e:
    print("next", e.code)
# (c) synchronous calls are not affected by the device word
print("dropin", rpc_amd.rpc_crc32(b"123456789") == 0xCBF43926)
print("host2", bool(np.array_equal(rpc_amd.crc32_batch(big, offs, lens), want_big)))
# (d) clear: asynchronous calls work again, every CRC exact
print("clear", rpc_amd.device_clear_status(), rpc_amd.device_status())
got = rpc_amd.device_uniform(base, n, L).cpu().numpy().view(np.uint32)
print("after_clear", bool(np.array_equal(got, oracle.crc32_uniform(base.cpu().numpy(), n, L))))
"""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RPCCRC_TEST_STEAL_GIVEUP="2", PYTHONPATH=repo,
               RPCCRC_LIB=os.path.join(repo, "rpc_amd", "lib", "librpccrc_test.so"))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=180, env=env, cwd=repo)
    assert p.returncode == 0, p.stderr[-3000:]
    out = p.stdout
    for want in ("host1 -5", "status_after_host 0", "status -5", "next -5", "dropin True", "host2 True",
                 "clear -5 0", "after_clear True"):
        assert want in out, (want, out)


def test_drop_in_frames(golden):
    """The captured wire frames: header CRC == rpc_crc32(body)."""
    for f in golden["frames"]:
        hdr = bytes.fromhex(f["header_hex"])
        body = f["body"].encode()
        assert rpc_amd.rpc_crc32_verify(body, int.from_bytes(hdr[8:12], "big"))


def test_drop_in_one_wave_kernel_lengths():
    """Bodies <= 4 KiB take the one-wave scalar kernel (crc32_scalar.hip): every
    length 0..1100, every segment-size boundary up to 4 KiB and past it (rows
    path), each right after a 4 KiB body of 0xFF so stale staging bytes before
    the body must be masked."""
    lens = list(range(0, 1101)) + [b + d for b in (2048, 4096) for d in (-65, -64, -63, -1, 0, 1, 63, 64, 65)]
    lens += [65535, 65536, 65537]
    ff = b"\xff" * 4096
    want_ff = oracle.crc32(ff)
    for n in lens:
        data = oracle.splitmix_bytes(n, 0x5CA1 + n) if n else b""
        assert rpc_amd.rpc_crc32(ff) == want_ff
        assert rpc_amd.rpc_crc32(data) == oracle.crc32(data), n


def test_drop_in_thread_safety():
    rng = np.random.default_rng(3)
    bodies = [rng.integers(0, 256, int(rng.integers(0, 3000)), dtype=np.uint8).tobytes() for _ in range(400)]
    want = [oracle.crc32(b) for b in bodies]
    errors = []

    def worker(k):
        for i in range(k, len(bodies), 8):
            if rpc_amd.rpc_crc32(bodies[i]) != want[i]:
                errors.append(i)

    th = [threading.Thread(target=worker, args=(k,)) for k in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors


def test_drop_in_service_stress_inline_boundary():
    """The drop-in service's request blocks (crc32_kernels.h SvcReq): bodies of up
    to 116 B travel inline in two request lines validated by a tag, longer ones in
    the body area.  10 threads x 3000 back-to-back calls on their slots, lengths
    0..240 around the inline bound, each body differing from the slot's previous
    one, every CRC against the oracle (a torn or stale line would show)."""
    rng = np.random.default_rng(17)
    pool = rng.integers(0, 256, 1 << 16, dtype=np.uint8).tobytes()
    errors = []

    def worker(k):
        r = np.random.default_rng(100 + k)
        for _ in range(3000):
            L = int(r.integers(0, 241))
            o = int(r.integers(0, len(pool) - L))
            b = pool[o:o + L]
            if rpc_amd.rpc_crc32(b) != oracle.crc32(np.frombuffer(b, dtype=np.uint8)):
                errors.append((k, L))

    th = [threading.Thread(target=worker, args=(k,)) for k in range(10)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[:10]


def _json_rpc_pair_bodies(k, n):
    """n JSON-RPC request bodies (client/rpc_codec.c:17's unformatted cJSON shape) for
    caller k: in pairs of one length whose id and first parameter step together, so
    consecutive bodies on a slot differ in two dwords by the same XOR delta whenever
    the two digits share a byte lane; inline (<= 116 B) and body-area (117 B -- 1 KiB)
    pairs alternate."""
    out = []
    for i in range(n):
        run = i // 2
        d = 1 + (i + k) % 9
        pad = 80 + (run * 37 + k) % 900 if run & 1 else (run * 13 + k) % 40
        shift = (run // 2 + k) % 4
        s = ('{"jsonrpc":"2.0","method":"add","params":[%d,"%s","%s"],"id":%d}'
             % (d, "x" * shift, "".join(chr(97 + (j * 7) % 26) for j in range(pad)), d))
        out.append(s.encode()[:1024])
    return out


def test_drop_in_service_json_pairs_stress():
    """10 threads x 3000 drop-in calls each, every caller on its
    own slot, with the bodies the reference actually checksums -- JSON-RPC requests
    (client/rpc_codec.c:17, stamped at rpc_async.c:525, verified at
    rpc_server_main.c:227) whose id and first parameter step together, so consecutive
    bodies on a slot differ in two dwords by equal XOR deltas, inline and body-area
    lengths alternating.  Every CRC against the oracle (the service's check must
    reject any torn read of such a pair; tests/cpu_emu/svc_check_emu.cpp proves the
    rule on the CPU, this runs it over PCIe)."""
    errors = []
    bodies = [_json_rpc_pair_bodies(k, 3000) for k in range(10)]
    wants = [[oracle.crc32(b) for b in bb] for bb in bodies]
    assert any(len(b) <= 116 for b in bodies[0]) and any(len(b) > 116 for b in bodies[0])
    before = rpc_amd.service_stats()

    def worker(k):
        for b, w in zip(bodies[k], wants[k]):
            if rpc_amd.rpc_crc32(b) != w:
                errors.append((k, len(b)))

    th = [threading.Thread(target=worker, args=(k,)) for k in range(10)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    st = rpc_amd.service_stats()
    print("service answered", st["answered"] - before["answered"], "of 30000 calls")
    assert not errors, errors[:10]
    # (a call finding all 16 slots held launches a kernel instead; 10 callers fit)
    assert st["answered"] - before["answered"] >= 29000, (before, st)


# ---- device batches ------------------------------------------------------------

@pytest.mark.parametrize("body_len", [1, 3, 4, 15, 16, 17, 63, 64, 100, 1000, 1023, 1024, 1025, 2000, 4080,
                                      4095, 4096, 4097, 4100, 8192, 12345, 65536])
@pytest.mark.parametrize("pad", [0, 7])
def test_device_uniform(body_len, pad):
    stride = body_len + pad
    n = max(1, min(3000, (6 << 20) // stride))
    host = oracle.splitmix_bytes(n * stride + 16, body_len * 31 + pad)
    base = to_dev(host)
    got = u32(rpc_amd.device_uniform(base, n, body_len, stride))
    assert np.array_equal(got, oracle.crc32_uniform(host, n, body_len, stride))


@pytest.fixture(params=["rows", "packed", "split"])
def ragged_path(request):
    """Both ragged-batch kernels: one wavefront per body, and 1 KiB chunks packed four per row."""
    rpc_amd.set_ragged_path(request.param)
    yield request.param
    rpc_amd.set_ragged_path("auto")


def _ragged_check(host, offs, lens):
    got = u32(rpc_amd.device_batch(to_dev(host), to_dev(offs.view(np.int64)), to_dev(lens.view(np.int32))))
    want = oracle.crc32_batch(host, offs, lens)
    if not np.array_equal(got, want):
        bad = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"body {bad} (len {int(lens[bad])}, off {int(offs[bad])}): "
                             f"{got[bad]:08x} != {want[bad]:08x}")


def _packed_offsets(lens, misalign):
    return (np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]) + misalign).astype(np.uint64)


@pytest.mark.parametrize("misalign", [0, 1, 3, 8, 13])
def test_device_batch_ragged(misalign, ragged_path):
    rng = np.random.default_rng(100 + misalign)
    lens = rng.integers(0, 70000, 600).astype(np.uint32)
    lens[::37] = 0
    lens[5] = 1
    lens[6] = 65536
    offs = _packed_offsets(lens, misalign)
    host = oracle.splitmix_bytes(int(lens.sum()) + misalign + 16, 77 + misalign)
    _ragged_check(host, offs, lens)


def test_device_batch_unordered_overlapping(ragged_path):
    """Offsets in any order, bodies may overlap (each is an independent view)."""
    rng = np.random.default_rng(9)
    host = oracle.splitmix_bytes(1 << 20, 5)
    lens = rng.integers(0, 20000, 500).astype(np.uint32)
    offs = rng.integers(0, (1 << 20) - 20000, 500).astype(np.uint64)
    _ragged_check(host, offs, lens)


@pytest.mark.parametrize("misalign", [0, 5])
def test_device_batch_tiny_bodies(misalign, ragged_path):
    """Up to four bodies per 4 KiB row in the packed kernel, every pad z = 0..15."""
    rng = np.random.default_rng(31 + misalign)
    lens = rng.integers(0, 90, 20000).astype(np.uint32)
    lens[::11] = 0
    offs = _packed_offsets(lens, misalign)
    host = oracle.splitmix_bytes(int(lens.sum()) + misalign + 16, 8 + misalign)
    _ragged_check(host, offs, lens)


def test_device_batch_chunk_boundaries(ragged_path):
    """Lengths around the 1 KiB chunk and 4 KiB row boundaries, at every misalignment
    (and the rows kernel's quarter / half first rows: first-row bytes incl. pad <= 1024 / 2048)."""
    base_lens = [1008, 1009, 1016, 1023, 1024, 1025, 1040, 2032, 2033, 2047, 2048, 2049, 2064, 3071, 3072, 3073,
                 4095, 4096, 4097, 5104, 5105, 5119, 5120, 6128, 6129, 6143, 6144, 6145, 8191, 8192, 8193]
    lens = np.array([L for L in base_lens for _ in range(16)] * 3, dtype=np.uint32)
    offs = np.empty(len(lens), dtype=np.uint64)
    pos = 0
    for i, L in enumerate(lens):
        pos += i % 16  # every end alignment
        offs[i] = pos
        pos += int(L)
    host = oracle.splitmix_bytes(pos + 16, 12)
    _ragged_check(host, offs, lens)


def test_device_batch_long_and_short_mix(ragged_path):
    """Slices that start inside long bodies (the wave owning the body's first chunk
    runs past its slice end) next to runs of tiny and empty bodies."""
    pattern = [65536, 1, 2, 3, 70001, 0, 0, 5000, 16, 0, 262147, 7]
    lens = np.array(pattern * 60, dtype=np.uint32)
    offs = _packed_offsets(lens, 3)
    host = oracle.splitmix_bytes(int(lens.sum()) + 32, 13)
    _ragged_check(host, offs, lens)


def test_device_batch_all_empty(ragged_path):
    lens = np.zeros(300, dtype=np.uint32)
    lens[150] = 1
    offs = np.arange(300, dtype=np.uint64)
    host = oracle.splitmix_bytes(512, 14)
    _ragged_check(host, offs, lens)
    lens[150] = 0
    _ragged_check(host, offs, lens)


@pytest.mark.parametrize("n,body_len,stride", [(65536 + 12345, 1500, 1500), (262144 + 4321, 200, 203),
                                                (65536 * 2 + 31, 4096, 4096),
                                                # QB = 4 affine metadata (stride % 4 == 0): pads z_b
                                                # alternate 0/8 across quarters; last group partial
                                                (262144 + 77, 1000, 1000), (262144 + 5, 500, 508),
                                                (262144 + 2, 1024, 1024)])
def test_device_uniform_workgroup_dynamic(n, body_len, stride):
    """Batches large enough for the workgroup-dynamic dealing (>= 8 rounds of 32
    tasks per workgroup), with a partial last round and pads z != 0."""
    host = oracle.splitmix_bytes(n * stride + 16, n ^ body_len)
    got = u32(rpc_amd.device_uniform(to_dev(host), n, body_len, stride))
    want = oracle.crc32_uniform(host, n, body_len, stride)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} mismatches, first body {int(bad[0])}"


def test_device_batch_rows_workgroup_dynamic():
    """The rows kernel on a large ragged batch (one wave per body, dynamic dealing)."""
    rng = np.random.default_rng(71)
    lens = rng.integers(0, 3000, 70001).astype(np.uint32)
    offs = _packed_offsets(lens, 9)
    host = oracle.splitmix_bytes(int(lens.sum()) + 32, 15)
    rpc_amd.set_ragged_path("rows")
    try:
        _ragged_check(host, offs, lens)
    finally:
        rpc_amd.set_ragged_path("auto")


@pytest.mark.parametrize("misalign", [0, 7])
def test_device_batch_split_workgroup_dynamic(misalign):
    """The split path on a large ragged batch: small bodies (<= 1 KiB with their
    end pad, incl. 1009..1024 B bodies that fit or not by alignment) four per
    row through the QB = 4 kernel with dynamic dealing, the rest through QB = 1,
    both writing through the index lists; unordered and empty bodies."""
    rng = np.random.default_rng(72 + misalign)
    n = 300007
    lens = np.where(rng.random(n) < 0.5, rng.integers(0, 1025, n), rng.integers(1000, 9000, n)).astype(np.uint32)
    lens[::97] = 0
    offs = _packed_offsets(lens, misalign)
    perm = rng.permutation(n)  # batch order differs from memory order
    host = oracle.splitmix_bytes(int(lens.sum()) + 64, 16)
    rpc_amd.set_ragged_path("split")
    try:
        _ragged_check(host, offs[perm].copy(), lens[perm].copy())
    finally:
        rpc_amd.set_ragged_path("auto")


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 33, 4095, 65536 + 5])
def test_split_small_body_kernel_counts(n):
    """The split path's small-body kernel (crc32_small.h): a wave walks whole
    iterations of 16 bodies of its list range, so counts that are not multiples
    of 16, lists shorter than one wave's share and lists much shorter than the
    batch (the grid is sized for the batch) all have to come out exact.  Bodies
    of 0..1024 B at every 16-B phase (those whose end pad pushes them past 1 KiB
    go to the other list), a few large ones mixed in; unordered offsets."""
    rng = np.random.default_rng(4000 + n)
    lens = rng.integers(0, 1025, n).astype(np.uint32)
    lens[::11] = 0
    big = rng.random(n) < 0.1
    lens[big] = rng.integers(1025, 20000, int(big.sum()))
    gaps = rng.integers(0, 16, n).astype(np.uint64)
    offs = (np.concatenate([[0], np.cumsum(lens[:-1].astype(np.uint64) + gaps[:-1])]) + gaps[0]).astype(np.uint64)
    perm = rng.permutation(n)
    host = oracle.splitmix_bytes(int(offs[-1]) + int(lens[-1]) + 32, 4000 + n)
    rpc_amd.set_ragged_path("split")
    try:
        _ragged_check(host, offs[perm].copy(), lens[perm].copy())
    finally:
        rpc_amd.set_ragged_path("auto")


def test_ragged_path_option():
    with pytest.raises(rpc_amd.RpcCrcError):
        rpc_amd.set_ragged_path(7)
    rpc_amd.set_ragged_path("auto")


def test_device_golden_random_bodies(golden):
    rb = golden["random_bodies"]
    parts = [oracle.splitmix_bytes(r["len"], r["seed"]) for r in rb]
    lens = np.array([r["len"] for r in rb], dtype=np.uint32)
    offs = (np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]) + 3).astype(np.uint64)
    host = np.concatenate([np.zeros(3, np.uint8)] + parts + [np.zeros(16, np.uint8)])
    got = u32(rpc_amd.device_batch(to_dev(host), to_dev(offs.view(np.int64)), to_dev(lens.view(np.int32))))
    assert got.tolist() == [r["crc"] for r in rb]


def test_device_json_c0(golden):
    """Config C0: 1024 x 4 KiB JSON-RPC bodies (the reference's CPU case) on the device."""
    buf, offs, lens = oracle.json_bodies(1024, 4096, 0x5EED0001)
    got = u32(rpc_amd.device_uniform(to_dev(buf), 1024, 4096))
    assert np.array_equal(got, oracle.crc32_batch(buf, offs, lens))
    assert got[:16].tolist() == golden["json_c0"]["crcs"]


@pytest.mark.parametrize("chunk", [0, 256, 1024, 65536, 4096 + 16])
def test_device_large(chunk):
    """Bodies with gaps between them: the chunk-table (expand) path; chunk 256
    gives the 33 MiB body > 64Ki chunks (several combine blocks per body)."""
    lens = [0, 1, 17, 4096, (5 << 20) + 3, (33 << 20) + 11]
    offs, pos = [], 5
    for L in lens:
        offs.append(pos)
        pos += L + 3
    host = oracle.splitmix_bytes(pos + 16, 1234)
    got = u32(rpc_amd.device_large(to_dev(host), offs, lens, chunk=chunk))
    want = [oracle.crc32(host[o:o + L]) for o, L in zip(offs, lens)]
    assert got.tolist() == want


@pytest.mark.parametrize("chunk,lens", [
    (0, [16384, 0, 3 * 16384, (5 << 20), 16384 * 7]),      # default chunk 16 KiB, one empty body
    (0, [4096 * 3, 8192, (1 << 20) + 4096]),               # default picks 4 KiB (lengths not multiples of 8 KiB)
    (0, [8192 * 5, (2 << 20) + 8192]),                     # default picks 8 KiB
    (4096, [4096] * 32),                                   # 32 bodies: the inline-table limit
    (1024 + 16, [1040 * 3, 1040 * 100, 0, 1040]),          # chunk not a power of two
    (256, [(17 << 20)]),                                   # > 64Ki chunks: falls back to the chunk table
])
def test_device_large_contiguous(chunk, lens):
    """Back-to-back bodies whose lengths are multiples of the chunk: the uniform
    fast path (one uniform rows launch + combine, no chunk table), at an odd base."""
    offs, pos = [], 5
    for L in lens:
        offs.append(pos)
        pos += L
    host = oracle.splitmix_bytes(pos + 16, 4321)
    got = u32(rpc_amd.device_large(to_dev(host), offs, lens, chunk=chunk))
    want = [oracle.crc32(host[o:o + L]) for o, L in zip(offs, lens)]
    assert got.tolist() == want
    # 33 bodies (one past the inline table) with the same layout rule
    if len(lens) == 32:
        lens2 = lens + [4096]
        offs2 = [5 + 4096 * i for i in range(33)]
        host2 = oracle.splitmix_bytes(5 + 4096 * 33 + 16, 99)
        got2 = u32(rpc_amd.device_large(to_dev(host2), offs2, lens2, chunk=chunk))
        assert got2.tolist() == [oracle.crc32(host2[o:o + L]) for o, L in zip(offs2, lens2)]


@pytest.mark.parametrize("chunk,blen,nb,gap", [
    (256, 4 << 20, 3, 0),    # 16Ki chunks per body: contiguous-run combine, M = 16
    (256, 8 << 20, 2, 0),    # M = 32
    (1024, 64 << 20, 2, 0),  # M = 64 (C4's shape at 4 KiB chunks: 64Ki chunks per body)
    (256, 4 << 20, 3, 3),    # gaps between bodies: chunk-table path, same combine when aligned
])
def test_device_large_equal_bodies_combine(chunk, blen, nb, gap):
    """Equal bodies of 1024 * M power-of-two chunks take crc32_chunk_combine_contig_kernel."""
    offs = [5 + i * (blen + gap) for i in range(nb)]
    host = oracle.splitmix_bytes(offs[-1] + blen + 16, 777 + blen + gap)
    got = u32(rpc_amd.device_large(to_dev(host), offs, [blen] * nb, chunk=chunk))
    assert got.tolist() == [oracle.crc32(host[o:o + blen]) for o in offs]


@pytest.mark.parametrize("blen,nb,misalign", [
    (16 << 20, 16, 0),   # 64Ki one-row chunks: the smallest batch with round values on 256 CUs
    (48 << 20, 6, 16),   # S = 3 (384 round values per body)
    (256 << 20, 1, 0),   # one C4 body (S = 16: 2048 round values)
    (256 << 20, 1, 3),   # misaligned base (trailing pads 13): per-chunk fold
    (48 << 20, 6, 5),    # misaligned base (pads 11): per-chunk fold
    (16 << 20, 8, 0),    # 32Ki chunks: too few rounds per workgroup, per-chunk fold
])
def test_device_large_round_values(blen, nb, misalign):
    """Back-to-back equal bodies of a multiple of 16 MiB (4 KiB chunks): the rows
    pass also stores each 32-chunk round's crc0 (ItemsArgs.round_out, a lane tree
    over the image's round maps) and the contiguous combine folds those.  Bases
    that are not 16-byte aligned keep the per-chunk fold (the round maps share
    the image slots of trailing pads 12..15)."""
    base = torch.empty((misalign + nb * blen + 16 + 7) // 8 * 8, dtype=torch.uint8, device=DEV)
    rpc_amd.fill_random(base, 0x20D0 + nb)
    offs = [misalign + i * blen for i in range(nb)]
    got = u32(rpc_amd.device_large(base, offs, [blen] * nb))
    torch.cuda.synchronize()
    assert rpc_amd.device_status() == 0
    want = oracle.crc32_batch_mt(base.cpu().numpy(), np.array(offs, dtype=np.uint64),
                                 np.full(nb, blen, dtype=np.uint64))
    assert got.tolist() == want.tolist()


def test_tail_stealing_back_to_back_launches():
    """Uniform one-row batches deal their last rounds from a leased device counter
    that each launch's last workgroup resets (crc32_rows.h kStealAhead).  70
    launches back to back on one stream cycle through the counter slots (64 per
    pool chunk), two streams interleave, and every launch must produce every CRC."""
    n, L = 65536, 4096  # the smallest batch that deals dynamically on 256 CUs
    host = oracle.splitmix_bytes(n * L, 0x57EA1)
    base = to_dev(host)
    ref = u32(rpc_amd.device_uniform(base, n, L))
    assert np.array_equal(ref, oracle.crc32_uniform_mt(host, n, L))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for k in range(70):
        st = s1 if k % 3 else s2
        with torch.cuda.stream(st):
            outs.append(rpc_amd.device_uniform(base, n, L, stream=st))
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        assert np.array_equal(u32(o), ref), k


def test_nontemporal_option_same_result():
    host = oracle.splitmix_bytes(4096 * 500, 8)
    base = to_dev(host)
    a = u32(rpc_amd.device_uniform(base, 500, 4096))
    rpc_amd.set_options(nontemporal=True)
    try:
        b = u32(rpc_amd.device_uniform(base, 500, 4096))
    finally:
        rpc_amd.set_options(nontemporal=False)
    assert np.array_equal(a, b)


def test_fill_random_matches_oracle_stream():
    t = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    rpc_amd.fill_random(t, 0x5EED0003)
    assert np.array_equal(t.cpu().numpy(), oracle.splitmix_bytes(1 << 20, 0x5EED0003))


# ---- host-buffer batch API --------------------------------------------------------

@pytest.mark.parametrize("pinned", [False, True])
def test_host_batch(pinned):
    rng = np.random.default_rng(21)
    lens = rng.integers(0, 40000, 3000).astype(np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64) + 1
    host = oracle.splitmix_bytes(int(lens.sum()) + 32, 4)
    if pinned:
        pt = torch.from_numpy(host).pin_memory()
        host = pt.numpy()
    got = rpc_amd.crc32_batch(host, offs, lens)
    assert np.array_equal(got, oracle.crc32_batch(host, offs, lens))
    exp = got.copy()
    exp[::5] ^= 1
    bad, ok = rpc_amd.verify_batch(host, offs, lens, exp)
    assert bad == len(exp[::5]) and ok[1] == 1 and ok[0] == 0


def test_host_batch_spans_many_stages():
    """> 256 MiB stage: exercises the double-buffered H2D pipeline and the large-body path."""
    n, L = 80, 4 << 20
    host = np.empty(n * L + (300 << 20), dtype=np.uint8)
    host[: n * L] = np.tile(oracle.splitmix_bytes(L, 6), n)
    host[n * L:] = oracle.splitmix_bytes(300 << 20, 7)
    offs = np.array([i * L for i in range(n)] + [n * L], dtype=np.uint64)
    lens = np.array([L] * n + [300 << 20], dtype=np.uint32)
    got = rpc_amd.crc32_batch(host, offs, lens)
    c = oracle.crc32(host[:L])
    assert (got[:n] == c).all()
    assert got[n] == oracle.crc32(host[n * L:])


# ---- BASELINE.json full sizes: size-independent properties --------------------------

def _sample_check(base_dev, n, L, stride, got, k=1500, seed=0):
    rng = np.random.default_rng(seed)
    idx = rng.choice(n, size=min(k, n), replace=False)
    for i in idx:
        body = base_dev[int(i) * stride:int(i) * stride + L].cpu().numpy()
        assert got[i] == oracle.crc32(body), int(i)


def _linearity(n, L, seed_x, seed_y):
    x = torch.empty(n * L, dtype=torch.uint8, device=DEV)
    y = torch.empty_like(x)
    rpc_amd.fill_random(x, seed_x)
    rpc_amd.fill_random(y, seed_y)
    cx = u32(rpc_amd.device_uniform(x, n, L))
    cy = u32(rpc_amd.device_uniform(y, n, L))
    xy = torch.bitwise_xor(x, y)
    cxy = u32(rpc_amd.device_uniform(xy, n, L))
    zero = oracle.crc32(bytes(L))
    assert np.all((cx ^ cy ^ cxy) == zero)
    return x, cx


def test_north_star_1M_x_4KiB():
    n, L = 1 << 20, 4096
    x, cx = _linearity(n, L, 0x5EED0003, 0x5EED0013)
    _sample_check(x, n, L, L, cx)
    # checksum of checksums: the whole 4 GiB as one body == fold of per-body CRCs
    whole = u32(rpc_amd.device_large(x, [0], [n * L]))[0]
    acc = int(cx[0])
    for c in cx[1:]:
        acc = oracle.combine(acc, int(c), L)
    assert whole == acc


@pytest.mark.parametrize("n,L", [(1 << 20, 4096), (1 << 20, 1024), (3 << 18, 3000)])
def test_full_coverage_dynamic_dealing(n, L):
    """EVERY CRC of a full-size batch against the oracle: the workgroup-dynamic
    dealing at bench scale (north star, C1, and partial rows with z != 0).  A
    lost or duplicated round is 32 bodies in 1M, which a sampled check misses
    (a tail-dealing design once did exactly that)."""
    x = torch.empty(n * L, dtype=torch.uint8, device=DEV)
    rpc_amd.fill_random(x, n ^ L)
    got = u32(rpc_amd.device_uniform(x, n, L))
    want = oracle.crc32_uniform(x.cpu().numpy(), n, L)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} mismatches, first body {int(bad[0])}, rounds {sorted(set((bad // 32).tolist()))[:8]}"


def test_c1_1M_x_1KiB():
    n, L = 1 << 20, 1024
    x, cx = _linearity(n, L, 0x5EED0002, 0x5EED0012)
    _sample_check(x, n, L, L, cx, seed=1)


def test_c2_ragged_loguniform_sample():
    n = 1 << 19  # 1/8 of config C2's 4M bodies (same distribution), ~4.6 GiB
    lens = oracle.loguniform_lengths(n, 0x5EED0004)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    total = int(lens.sum())
    base = torch.empty(total + 8, dtype=torch.uint8, device=DEV)
    rpc_amd.fill_random(base, 0x5EED0004)
    doffs, dlens = to_dev(offs.view(np.int64)), to_dev(lens.view(np.int32))
    got = u32(rpc_amd.device_batch(base, doffs, dlens))  # auto: the rows kernel
    want = oracle.crc32_batch(base.cpu().numpy(), offs, lens)  # every body
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} mismatches, first body {int(bad[0])}"
    # every body: the ragged kernels agree
    for path in ("packed", "split"):
        rpc_amd.set_ragged_path(path)
        try:
            other = u32(rpc_amd.device_batch(base, doffs, dlens))
        finally:
            rpc_amd.set_ragged_path("auto")
        assert np.array_equal(got, other), path


def _check_ragged_slices(base, offs, lens, got, slice_bytes=4 << 30):
    """Every CRC of a contiguous ragged batch against the threaded oracle, copying
    the device bytes back ~slice_bytes at a time."""
    ends = np.cumsum(lens, dtype=np.uint64)
    lo = 0
    n = lens.size
    while lo < n:
        hi = int(np.searchsorted(ends, np.uint64(int(offs[lo]) + slice_bytes), side="right"))
        hi = max(hi, lo + 1)
        b0, b1 = int(offs[lo]), int(offs[hi - 1]) + int(lens[hi - 1])
        part = base[b0:b1].cpu().numpy()
        want = oracle.crc32_batch_mt(part, offs[lo:hi] - np.uint64(b0), lens[lo:hi])
        bad = np.flatnonzero(got[lo:hi] != want)
        assert bad.size == 0, f"{bad.size} mismatches, first body {lo + int(bad[0])}, rounds " \
                              f"{sorted(set(((lo + bad) // 32).tolist()))[:8]}"
        del part
        lo = hi


def test_c2_full_size_every_crc():
    """config C2 at its BASELINE size -- 4M bodies, log-uniform
    64 B - 64 KiB (seed 0x5EED0004), ~37 GiB back to back, exactly the bench's
    workload (bench.py Workload "c2": the bounded call with max_len = 64 KiB) --
    EVERY CRC against the oracle (reference crc.c:4-9 body by body), in ~4 GiB
    slices.  The ragged DYN launch deals 8x the rounds of the 1/8 sample; a lost
    or duplicated round is 32 bodies, which a sample misses.  The unbounded call
    (route classify + empty route passes) must give the same outputs."""
    n = 1 << 22
    lens = oracle.loguniform_lengths(n, 0x5EED0004)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    total = int(lens.sum(dtype=np.uint64))
    base = torch.empty((total + 15) // 8 * 8, dtype=torch.uint8, device=DEV)
    rpc_amd.fill_random(base, 0x5EED0004)
    doffs, dlens = to_dev(offs.view(np.int64)), to_dev(lens.view(np.int32))
    got = u32(rpc_amd.device_batch(base, doffs, dlens, max_len=int(lens.max())))
    plain = u32(rpc_amd.device_batch(base, doffs, dlens))
    assert np.array_equal(got, plain)
    _check_ragged_slices(base, offs, lens, got)
    assert rpc_amd.device_status() == 0


def _dense_case(lens, pad=0, gap_at=None, seed=0xDE45, max_len=None):
    """A batch of bodies back to back from byte `pad` of a buffer (a gap of 16 B
    before body gap_at, if given), every CRC through the bounded call against the
    oracle, and against the unbounded call (rows + route: no dense plan)."""
    lens = np.asarray(lens, dtype=np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64) + np.uint64(pad)
    if gap_at is not None:
        offs[gap_at:] += np.uint64(16)
    total = int(offs[-1]) + int(lens[-1])
    # (at most 7 B of tail room, for fill_random's 8-B words: the span's last
    # block is range-checked at the stream's 16-B end)
    base = torch.empty((total + 7) // 8 * 8, dtype=torch.uint8, device=DEV)
    rpc_amd.fill_random(base, seed)
    doffs, dlens = to_dev(offs.view(np.int64)), to_dev(lens.view(np.int32))
    got = u32(rpc_amd.device_batch(base, doffs, dlens, max_len=int(lens.max()) if max_len is None else max_len))
    torch.cuda.synchronize()
    host = base.cpu().numpy()
    want = oracle.crc32_batch_mt(host, offs, lens)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:10], lens[bad[:10]])
    plain = u32(rpc_amd.device_batch(base, doffs, dlens))
    assert np.array_equal(got, plain)
    assert rpc_amd.device_status() == 0


@pytest.mark.parametrize("case", ["loguniform", "tiny_dense", "block_ends", "pad7", "max_body", "mixed_runs"])
def test_dense_span_mode(case):
    """a bounded ragged batch whose bodies lie back to back in order,
    each of 64 B - 1 MiB, takes the dense span pass (uniform 4 KiB blocks of the
    whole stream + per-boundary values + a per-body fold).  Every CRC against the
    oracle and against the rows path: log-uniform 64 B - 64 KiB (C2's shape), runs
    of 64-100 B bodies (> 6 boundaries a block: the record's overflow path), bodies
    ending exactly on block boundaries (and the stream's end on one), a stream
    starting 7 B into its buffer (the anchor rounds down to 16 B), 240 KiB bodies (the
    longest a bounded batch sends through the step: a bound of 256 KiB or more takes the
    big-body route) and alternating runs of tiny and large bodies."""
    rng = np.random.default_rng(hash(case) & 0xFFFF)
    n = 1 << 17
    if case == "loguniform":
        lens = oracle.loguniform_lengths(n, 0xD0E5)
        _dense_case(lens)
    elif case == "tiny_dense":  # (4M bodies: the step needs >= 8 DYN rounds of blocks per workgroup)
        _dense_case(rng.integers(64, 101, 1 << 22).astype(np.uint32))
    elif case == "block_ends":
        lens = np.full(n, 4096, dtype=np.uint32)
        lens[0::3] = 4032
        lens[1::3] = 64
        lens[2::3] = 8192
        _dense_case(lens)
    elif case == "pad7":
        _dense_case(rng.integers(64, 5000, n).astype(np.uint32), pad=7)
    elif case == "max_body":  # (60-block bodies; a bound >= 256 KiB takes the big-body route instead)
        lens = rng.integers(64, 3000, n).astype(np.uint32)
        lens[::997] = 240 << 10
        _dense_case(lens)
    else:
        lens = np.where((np.arange(n) // 500) % 2 == 0, rng.integers(64, 128, n),
                        rng.integers(20000, 65537, n)).astype(np.uint32)
        _dense_case(lens)


@pytest.mark.parametrize("case", ["gap", "short_body", "long_body", "unordered", "reversed"])
def test_dense_plan_falls_back(case):
    """A bounded ragged batch the dense plan must refuse -- a 16-B gap between two
    bodies, a 63-B body, a body over 1 MiB, bodies out of order, the whole batch in
    reverse (every offset below the first body's: stream offsets that wrap, which
    the plan must not use to write records) -- is CRC'd by the rows pass instead
    (decided on the device): every CRC against the oracle."""
    rng = np.random.default_rng(7)
    n = 1 << 17
    lens = rng.integers(64, 3000, n).astype(np.uint32)
    if case == "gap":
        _dense_case(lens, gap_at=n // 2)
    elif case == "short_body":
        lens[n // 3] = 63
        _dense_case(lens)
    elif case == "long_body":  # (a bound below the truth: results never depend on it)
        lens[n // 3] = (1 << 20) + 1
        _dense_case(lens, max_len=65536)
    else:
        offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
        perm = np.arange(n)
        if case == "unordered":
            perm[[10, 11]] = perm[[11, 10]]
        else:
            perm = perm[::-1].copy()
        offs, lens2 = offs[perm].copy(), lens[perm].copy()
        total = int(lens.sum(dtype=np.uint64))
        base = torch.empty((total + 7) // 8 * 8, dtype=torch.uint8, device=DEV)
        rpc_amd.fill_random(base, 0xABCD)
        got = u32(rpc_amd.device_batch(base, to_dev(offs.view(np.int64)), to_dev(lens2.view(np.int32)),
                                       max_len=int(lens.max())))
        torch.cuda.synchronize()
        want = oracle.crc32_batch_mt(base.cpu().numpy(), offs, lens2)
        assert np.array_equal(got, want)


def test_dense_mode_covers_every_crc():
    """The dense span step computes EVERY CRC of a dense batch by itself, and the
    plan refuses a batch that is not dense -- not just "the right
    answers come back", which the plain rows pass behind the plan would also give.
    In a child process on the test build with RPCCRC_TEST_DENSE_ONLY=1 that rows
    pass is left out: the output starts poisoned, every CRC of four dense layouts
    must then come from the span pass and the fold (oracle; 64-100 B bodies: 4M
    of them, for the >= 8 DYN rounds of blocks per workgroup the step needs),
    and a batch with a 16-B gap, or too small for the step, must leave the
    output untouched."""
    import os
    import subprocess
    import sys
    code = r"""
import numpy as np, torch, rpc_amd
from oracle import oracle
torch.cuda.set_device(0)
POISON = -0x5A5A5A5B  # 0xA5A5A5A5
def case(lens, pad=0, gap_at=None, seed=0xD1, bound=None):
    lens = np.asarray(lens, dtype=np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64) + np.uint64(pad)
    if gap_at is not None:
        offs[gap_at:] += np.uint64(16)
    total = int(offs[-1]) + int(lens[-1])
    base = torch.empty((total + 7) // 8 * 8, dtype=torch.uint8, device="cuda:0")
    rpc_amd.fill_random(base, seed)
    out = torch.full((lens.size,), POISON, dtype=torch.int32, device="cuda:0")
    rpc_amd.device_batch(base, torch.from_numpy(offs.view(np.int64)).cuda(), torch.from_numpy(lens.view(np.int32)).cuda(),
                         out=out, max_len=int(lens.max()) if bound is None else bound)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    return got, oracle.crc32_batch_mt(base.cpu().numpy(), offs, lens)
rng = np.random.default_rng(0xD0)
n = 1 << 17
for name, lens, pad in [("loguniform", oracle.loguniform_lengths(n, 0xD0E6), 0),
                        ("tiny", rng.integers(64, 101, 1 << 22), 0),
                        ("pad9", rng.integers(64, 9000, n), 9),
                        # bodies of 60 blocks (the fold's A_{65536 k} maps; a bound >= 256 KiB would
                        # send the batch through the big-body route instead)
                        ("max_body", np.where(np.arange(n) % 997 == 0, 240 << 10, rng.integers(64, 3000, n)), 0),
                        # the bound allows the step, the stream is small (2.1K blocks, counted on the device)
                        ("small_stream", np.where(np.arange(n) == 5, 240 << 10, 64), 3)]:
    got, want = case(lens, pad)
    print(name, int(np.count_nonzero(got != want)))
# the plain (unbounded) call, and a bound over the big-body route's threshold
# with 300 KiB bodies: the route's classify pass leaves every body to the step
got, want = case(oracle.loguniform_lengths(n, 0xD0E7), bound=0)
print("unbounded", int(np.count_nonzero(got != want)))
got, want = case(np.where(np.arange(n) % 499 == 0, 300 << 10, rng.integers(64, 3000, n)), bound=1 << 20)
print("over_route_bound", int(np.count_nonzero(got != want)))
# unbounded, a stream longer than the workspace's 64 KiB-per-body estimate (2^16
# bodies of 100 KiB: 1.6M blocks against 1M): refused, so left to the rows pass
nb = 1 << 16
lens_b = np.full(nb, 100 << 10, dtype=np.uint32)
offs_b = np.arange(nb, dtype=np.uint64) * np.uint64(100 << 10)
base_b = torch.zeros(nb * (100 << 10), dtype=torch.uint8, device="cuda:0")
out_b = torch.full((nb,), POISON, dtype=torch.int32, device="cuda:0")
rpc_amd.device_batch(base_b, torch.from_numpy(offs_b.view(np.int64)).cuda(), torch.from_numpy(lens_b.view(np.int32)).cuda(),
                     out=out_b)
torch.cuda.synchronize()
print("over_cap_untouched", bool(torch.all(out_b == POISON).item()))
del base_b
got, want = case(rng.integers(64, 3000, n), gap_at=n // 2)
print("gap_untouched", bool(np.all(got == np.uint32(0xA5A5A5A5))))
# too small for the dense step (< 8 DYN rounds of 4 KiB blocks per workgroup): not taken
got, want = case(rng.integers(64, 101, n))
print("small_untouched", bool(np.all(got == np.uint32(0xA5A5A5A5))))
print("status", rpc_amd.device_status())
"""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RPCCRC_TEST_DENSE_ONLY="1", PYTHONPATH=repo,
               RPCCRC_LIB=os.path.join(repo, "rpc_amd", "lib", "librpccrc_test.so"))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240, env=env, cwd=repo)
    assert p.returncode == 0, p.stderr[-3000:]
    for want in ("loguniform 0", "tiny 0", "pad9 0", "max_body 0", "small_stream 0", "unbounded 0",
                 "over_route_bound 0", "over_cap_untouched True", "gap_untouched True",
                 "small_untouched True",
                 "status 0"):
        assert want in p.stdout, (want, p.stdout)


def test_dyn_ragged_batch_with_huge_unrouted_body():
    """a DYN-sized ragged batch whose length bound (64 KiB)
    keeps a 512 MiB body off the big-body route, so ONE wave walks it (~0.1-0.3 s)
    while its siblings run 8 rounds ahead and wait for its output-ring slot.  The
    wait must outlast it (round 3's 0.1 s spin cap reported a false EIO and lost
    the round): every CRC exact, device status clean."""
    n_small = 200000
    rng = np.random.default_rng(0xB16)
    lens = rng.integers(1, 4000, n_small).astype(np.uint32)
    big = 512 << 20
    pos = 1000  # early in the batch: its round is dealt first, the rest run past it
    lens = np.insert(lens, pos, np.uint32(big))
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    total = int(lens.sum(dtype=np.uint64))
    base = torch.empty((total + 15) // 8 * 8, dtype=torch.uint8, device=DEV)
    rpc_amd.fill_random(base, 0xB16B0D7)
    got = u32(rpc_amd.device_batch(base, to_dev(offs.view(np.int64)), to_dev(lens.view(np.int32)),
                                   max_len=64 << 10))
    torch.cuda.synchronize()
    assert rpc_amd.device_status() == 0
    _check_ragged_slices(base, offs, lens, got, slice_bytes=1 << 30)


def test_c4_large_bodies():
    n, L = 16, 256 << 20
    base = torch.empty(n * L, dtype=torch.uint8, device=DEV)
    rpc_amd.fill_random(base, 0x5EED0006)
    got = u32(rpc_amd.device_large(base, [i * L for i in range(n)], [L] * n))
    # every body against the oracle (crc.c:4-9, body by body; 4 GiB on 16 host threads)
    host = base.cpu().numpy()
    want = oracle.crc32_batch_mt(host, np.arange(n, dtype=np.uint64) * np.uint64(L), np.full(n, L, dtype=np.uint32))
    del host
    assert np.array_equal(got, want), [i for i in range(n) if got[i] != want[i]]
    # and a property: per-1MiB-chunk uniform CRCs folded with crc32_combine
    sub = 1 << 20
    per = u32(rpc_amd.device_uniform(base, n * (L // sub), sub))
    for i in range(n):
        acc = int(per[i * (L // sub)])
        for c in per[i * (L // sub) + 1:(i + 1) * (L // sub)]:
            acc = oracle.combine(acc, int(c), sub)
        assert got[i] == acc


# ---- big bodies inside ragged batches: the device-side chunk route ----

BIG = 256 << 10  # kBigMin


@pytest.mark.parametrize("path", ["auto", "split"])
@pytest.mark.parametrize("misalign", [0, 5])
def test_device_batch_big_bodies_route(path, misalign):
    """Bodies around and far above the 256 KiB route threshold, mixed with small and
    empty ones, unordered: every CRC against the oracle."""
    lens = [3, BIG - 1, BIG, BIG + 1, 0, (1 << 20) + 13, 17, (64 << 20) + 5, 1000, (9 << 20) - 16, 4096,
            (2 << 20), 5000, BIG + 4097]
    offs = (np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]) + misalign).astype(np.uint64)
    perm = np.random.default_rng(misalign).permutation(len(lens))
    lens_p = np.array(lens, dtype=np.uint32)[perm]
    offs_p = offs[perm]
    base = torch.empty((int(offs[-1]) + lens[-1] + 16 + 7) // 8 * 8, dtype=torch.uint8, device=DEV)
    rpc_amd.fill_random(base, 0xB16B0D1E + misalign)
    rpc_amd.set_ragged_path(path)
    try:
        got = u32(rpc_amd.device_batch(base, to_dev(offs_p.view(np.int64)), to_dev(lens_p.view(np.int32))))
    finally:
        rpc_amd.set_ragged_path("auto")
    host = base.cpu().numpy()
    want = oracle.crc32_batch(host, offs_p, lens_p).tolist()
    assert got.tolist() == want
    # rpc_crc32_device_batch_bounded: a bound under the route threshold skips the
    # route; a WRONG bound (bodies above it) still gives every exact CRC (one wave
    # per big body), and the unbounded C entry point agrees
    d_o, d_l = to_dev(offs_p.view(np.int64)), to_dev(lens_p.view(np.int32))
    rpc_amd.set_ragged_path(path)
    try:
        wrong = u32(rpc_amd.device_batch(base, d_o, d_l, max_len=70000))
        right = u32(rpc_amd.device_batch(base, d_o, d_l, max_len=max(lens)))
        plain = torch.empty(len(lens), dtype=torch.int32, device=DEV)
        assert rpc_amd._lib.rpc_crc32_device_batch(base.data_ptr(), d_o.data_ptr(), d_l.data_ptr(), len(lens),
                                                   plain.data_ptr(), rpc_amd._stream_handle(None)) == 0
    finally:
        rpc_amd.set_ragged_path("auto")
    assert wrong.tolist() == want and right.tolist() == want and u32(plain).tolist() == want


def test_device_batch_route_overflow_and_overlap():
    """More big bodies than the route holds (16384): the extra ones keep one wave each;
    overlapping bodies; the same buffer region listed many times."""
    n_big = 16384 + 37
    L = BIG + 48
    region = torch.empty(4 << 20, dtype=torch.uint8, device=DEV)
    rpc_amd.fill_random(region, 0x0FF10)
    rng = np.random.default_rng(9)
    offs = rng.integers(0, (4 << 20) - L, n_big).astype(np.uint64)
    lens = np.full(n_big, L, dtype=np.uint32)
    lens[::97] = rng.integers(0, 3000, lens[::97].size)  # small ones in between
    got = u32(rpc_amd.device_batch(region, to_dev(offs.view(np.int64)), to_dev(lens.view(np.int32))))
    want = oracle.crc32_batch_mt(region.cpu().numpy(), offs, lens)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} mismatches, first {int(bad[0])}"


def test_device_batch_route_chunk_growth():
    """More than kBigMaxChunks x 16 KiB of routed bytes: the plan doubles the chunk.
    Five 3.75 GiB bodies over one region (18.75 GiB routed), each checked against the
    large-body path and against the oracle on the CPU (all five,
    not one)."""
    L = (15 << 28)  # 3.75 GiB
    region = torch.empty(L + 64, dtype=torch.uint8, device=DEV)
    rpc_amd.fill_random(region, 0xC4C4)
    offs = np.array([0, 16, 0, 64, 16], dtype=np.uint64)
    lens = np.array([L, L, L - 16, L, L], dtype=np.uint32)
    got = u32(rpc_amd.device_batch(region, to_dev(offs.view(np.int64)), to_dev(lens.view(np.int32))))
    # reference values: the large-body path (16 KiB chunks, host table) per distinct body
    for o, ln, g in zip(offs, lens, got):
        want = u32(rpc_amd.device_large(region, [int(o)], [int(ln)], chunk=4096 + 16))[0]
        assert g == want, (int(o), int(ln))
    # and every one of them on the CPU (one oracle thread per body)
    host = region.cpu().numpy()
    want = oracle.crc32_batch_mt(host, offs, lens, threads=5)
    assert [int(g) for g in got] == [int(w) for w in want]


def _hip_runtime():
    """The HIP runtime torch loaded (the same copy librpccrc binds to)."""
    import ctypes
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("libamdhip64 not loaded")


class _RawStream:
    """A hipStream_t of our own, so the test can really destroy one."""

    def __init__(self, hip):
        import ctypes
        self.hip, h = hip, ctypes.c_void_p()
        assert hip.hipStreamCreate(ctypes.byref(h)) == 0
        self.cuda_stream = h.value

    def destroy(self):
        import ctypes
        assert self.hip.hipStreamDestroy(ctypes.c_void_p(self.cuda_stream)) == 0


def test_workspace_pool_stream_switches():
    """cached workspaces across stream switches, growth while earlier work is
    in flight, a destroyed stream, and the scalar path alternating with the batch path."""
    hip = _hip_runtime()
    n, L = 12, 9 << 20
    base = torch.empty(n * L, dtype=torch.uint8, device=DEV)
    rpc_amd.fill_random(base, 0x5EEDF00D)
    host = base.cpu().numpy()
    want = [oracle.crc32(host[i * L:(i + 1) * L]) for i in range(n)]
    torch.cuda.synchronize()
    s1, s2 = _RawStream(hip), _RawStream(hip)
    outs = []
    for stream, k, chunk in [(s1, 2, 0), (s2, 12, 4096), (s1, 6, 1024), (s2, 12, 256)]:
        o = torch.empty(k, dtype=torch.int32, device=DEV)
        rpc_amd.device_large(base, [i * L for i in range(k)], [L] * k, chunk=chunk, out=o, stream=stream)
        outs.append((o, k))
    s2.destroy()  # its last call may still be in flight; the pool must not care
    s3 = _RawStream(hip)
    o3 = torch.empty(n, dtype=torch.int32, device=DEV)
    rpc_amd.device_large(base, [i * L for i in range(n)], [L] * n, chunk=2048, out=o3, stream=s3)
    # ragged batches (split + route workspaces) on the same streams
    offs = np.arange(n, dtype=np.uint64) * np.uint64(L)
    lens = np.full(n, L, dtype=np.uint32)
    o4 = torch.empty(n, dtype=torch.int32, device=DEV)
    rpc_amd.device_batch(base, to_dev(offs.view(np.int64)), to_dev(lens.view(np.int32)), out=o4, stream=s1)
    assert hip.hipDeviceSynchronize() == 0
    for o, k in outs:
        assert u32(o).tolist() == want[:k]
    assert u32(o3).tolist() == want
    assert u32(o4).tolist() == want
    s1.destroy()
    s3.destroy()
    # drop-in rpc_crc32 (>= 8 MiB: chunked path) alternating with rpc_crc32_batch
    for i in range(3):
        assert rpc_amd.rpc_crc32(host[i * L:(i + 1) * L]) == want[i]
        assert rpc_amd.crc32_batch(host, offs, lens).tolist() == want
        assert rpc_amd.rpc_crc32(host[:100]) == oracle.crc32(host[:100])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_workspace_layout_edges(n):
    """Every call that carves several arrays out of one leased block (rpc_amd/csrc/workspace.h),
    at the counts where n, 2n, 4n or 8n bytes sit just under, on and just over a 256-byte
    step: the smallest shapes at which two mis-carved neighbours overlap.  Bodies of 1-300 B,
    one process, one stream; every CRC against the oracle, every verdict OK.  (At these sizes
    the scan's "tiled" setting still walks serially: the stream is shorter than one tile.)"""
    rng = np.random.default_rng(n)
    lens = rng.integers(1, 301, n).astype(np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    total = int(lens.sum())
    host = np.concatenate([oracle.splitmix_bytes((total + 7) // 8 * 8, 0xED6E + n),
                           oracle.splitmix_bytes(BIG + 8, 0xB16 + n)])
    want = oracle.crc32_batch(host, offs, lens)
    base, d_o, d_l = to_dev(host), to_dev(offs.view(np.int64)), to_dev(lens.view(np.int32))
    ok = [rpc_amd.FRAME_OK] * n
    try:
        # 1. the packed, split and rows workspaces
        for path in ("packed", "split", "rows"):
            rpc_amd.set_ragged_path(path)
            assert np.array_equal(u32(rpc_amd.device_batch(base, d_o, d_l)), want), path
        rpc_amd.set_ragged_path("auto")
        # 2. the route's workspace: one more body, over the threshold, unbounded
        offs_b = np.append(offs, np.uint64((total + 7) // 8 * 8))
        lens_b = np.append(lens, np.uint32(BIG + 1))
        got = u32(rpc_amd.device_batch(base, to_dev(offs_b.view(np.int64)), to_dev(lens_b.view(np.int32)), max_len=0))
        assert np.array_equal(got, oracle.crc32_batch(host, offs_b, lens_b))
        # 3. the gather fold's: every body cut into three segments (some empty), seeded
        cut1, cut2 = lens // 3, lens // 3 + lens // 2
        seg_off = np.stack([offs, offs + cut1, offs + cut2], axis=1).reshape(-1).astype(np.uint64)
        seg_len = np.stack([cut1, cut2 - cut1, lens - cut2], axis=1).reshape(-1).astype(np.uint32)
        seeds = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        seg_crc = oracle.crc32_batch(host, seg_off, seg_len)
        want_g = []
        for i in range(n):
            c = int(seeds[i])
            for s in range(3 * i, 3 * i + 3):
                c = oracle.combine(c, int(seg_crc[s]), int(seg_len[s]))
            want_g.append(c)
        got = u32(rpc_amd.device_gather(base, to_dev(seg_off.view(np.int64)), to_dev(seg_len.view(np.int32)),
                                        to_dev((3 * np.arange(n + 1)).astype(np.int64)),
                                        seed=to_dev(seeds.view(np.int32))))
        assert got.tolist() == want_g
        # 4. stamp, then verify, cap lifted: with the library's own verdict / CRC array and with the caller's
        f_off = (offs + np.uint64(12) * np.arange(n, dtype=np.uint64)).astype(np.uint64)
        blob = np.zeros(total + 12 * n, dtype=np.uint8)
        for o, b, ln in zip(f_off, offs, lens):
            blob[int(o) + 12:int(o) + 12 + int(ln)] = host[int(b):int(b) + int(ln)]
        d_f, sh = to_dev(f_off.view(np.int64)), rpc_amd._stream_handle(None)
        lift = rpc_amd.FRAMES_LIFT_CAP
        own = to_dev(blob)
        assert rpc_amd._lib.rpc_frames_stamp_device(own.data_ptr(), own.numel(), d_f.data_ptr(), d_l.data_ptr(), n, 1,
                                                    rpc_amd.RPC_TYPE_DATA, lift, None, sh) == 0
        v = torch.full((n,), 0xEE, dtype=torch.uint8, device=DEV)
        assert rpc_amd._lib.rpc_frames_verify_device(own.data_ptr(), own.numel(), d_f.data_ptr(), n,
                                                     rpc_amd.FRAMES_SERVER | lift, v.data_ptr(), None, sh) == 0
        assert v.cpu().tolist() == ok
        mine = to_dev(blob)
        assert rpc_amd.frames_stamp(mine, d_f, d_l, lift_cap=True).cpu().tolist() == ok
        assert torch.equal(mine, own)
        v, c = rpc_amd.frames_verify(mine, d_f, role="client", lift_cap=True)
        assert v.cpu().tolist() == ok and np.array_equal(u32(c), want)
        # 5. pack, then the fused scan of what it wrote, as the other side reads it
        nc = min(n, 7)
        conn = to_dev((np.arange(nc + 1) * n // nc).astype(np.int64))
        p = rpc_amd.frames_pack(base, d_o, d_l, conn_first=conn)
        assert p.total == total + 12 * n and p.verdict.cpu().tolist() == ok and np.array_equal(u32(p.crc), want)
        assert p.offsets.cpu().numpy().view(np.uint64).tolist() == f_off.tolist()
        cbf = p.conn_bytes_first
        for path in ("serial", "tiled"):
            rpc_amd.set_scan_path(path)
            r = rpc_amd.frames_scan(p.stream, cbf[:-1].contiguous(), (cbf[1:] - cbf[:-1]).contiguous(), role="client",
                                    verify=True, max_frames=n)
            assert r.nframes == n and torch.equal(r.frame_offsets, p.offsets), path
            assert torch.equal(r.conn_first, conn), path
            assert r.verdict.cpu().tolist() == ok and np.array_equal(u32(r.crc), want), path
    finally:
        rpc_amd.set_ragged_path("auto")
        rpc_amd.set_scan_path("auto")


def test_c3_per_rank_shard_full_coverage():
    """Config C3's per-GPU shard at full size: 8M x 4 KiB = 32 GiB on one GPU (rank 0's
    seed), EVERY CRC against the oracle (threaded, 4 GiB at a time)."""
    n, L = 1 << 23, 4096
    x = torch.empty(n * L, dtype=torch.uint8, device=DEV)
    rpc_amd.fill_random(x, 0x5EED0005)
    got = u32(rpc_amd.device_uniform(x, n, L))
    step = 1 << 20
    for lo in range(0, n, step):
        part = x[lo * L:(lo + step) * L].cpu().numpy()
        want = oracle.crc32_uniform_mt(part, step, L)
        bad = np.flatnonzero(got[lo:lo + step] != want)
        assert bad.size == 0, f"{bad.size} mismatches, first body {lo + int(bad[0])}"
        del part


@pytest.mark.parametrize("n,L", [(1 << 18, 4096), (1 << 20, 1024)])
def test_drop_in_service_beside_batches(n, L):
    """The drop-in service (crc32_service.hip, one resident workgroup with 476 B
    of LDS) must share the chip with the rows kernel's persistent grid (one
    155-159 KiB-LDS workgroup per CU): batches while another thread keeps the
    service busy run at about their normal time (a workgroup that could not be
    placed would take ~1.5x), and every CRC of both is exact.  1M x 1 KiB is the
    QB = 4 kernel, the largest LDS footprint (an 8-slot ring left no room:
    251 vs 161 us, profiles/r04za)."""
    import time
    x = torch.empty(n * L, dtype=torch.uint8, device=DEV)
    rpc_amd.fill_random(x, 0x5E7)
    want = oracle.crc32_uniform_mt(x.cpu().numpy(), n, L)
    bodies = [oracle.splitmix_bytes(k, 0xD0 + k) for k in (12, 68, 300, 1000, 1024)]
    wants = [oracle.crc32(b) for b in bodies]

    def timed(reps=20):
        # per-launch event pairs, enqueued behind ~1 ms of other batches so that
        # a caller thread slowed by the hammering thread (the GIL) does not open
        # gaps: the median launch is the kernel's own time
        s = torch.cuda.current_stream()
        for _ in range(6):
            rpc_amd.device_uniform(x, n, L)
        ev = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            out = rpc_amd.device_uniform(x, n, L)
            e1.record(s)
            ev.append((e0, e1))
        ev[-1][1].synchronize()
        assert np.array_equal(u32(out), want)
        return float(np.median([a.elapsed_time(b) for a, b in ev]))

    alone = min(timed() for _ in range(3))
    errors, calls = [], [0]
    stop = threading.Event()

    def hammer():
        while not stop.is_set():
            for b, w in zip(bodies, wants):
                if rpc_amd.rpc_crc32(b) != w:
                    errors.append(len(b))
                calls[0] += 1

    th = threading.Thread(target=hammer)
    th.start()
    try:
        time.sleep(0.05)
        busy = min(timed() for _ in range(3))
    finally:
        stop.set()
        th.join()
    print(f"rows batch alone {alone * 1e3:.1f} us, beside the drop-in service {busy * 1e3:.1f} us, "
          f"{calls[0]} drop-in calls")
    assert not errors, errors
    assert calls[0] > 100
    assert busy < 1.3 * alone, (alone, busy)


def test_drop_in_beside_a_long_kernel():
    """drop-in calls while another thread's batch holds the GPU for
    seconds -- one body of 4 GiB - 64 B walked by ONE wave (its length bound below
    the big-body route's threshold skips the route) -- must each return the oracle
    CRC (the reference server's verify, rpc_server_main.c:227, may run beside any
    other GPU work).  The long body's CRC is checked too (16 x 256 MiB pieces on the
    host, folded with crc32_combine)."""
    import time
    L = (1 << 32) - 64
    base = torch.empty(L, dtype=torch.uint8, device=DEV)
    rpc_amd.fill_random(base, 0x10B6)
    offs = torch.zeros(1, dtype=torch.int64, device=DEV)
    lens = torch.from_numpy(np.array([L], dtype=np.uint32).view(np.int32)).to(DEV)
    out = torch.empty(1, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    bodies = [oracle.splitmix_bytes(k, 0xD1 + k) for k in (12, 68, 300, 1024)]
    wants = [oracle.crc32(b) for b in bodies]
    t_kernel = [0.0]

    def long_batch():
        t0 = time.perf_counter()
        rpc_amd.device_batch(base, offs, lens, out=out, max_len=65536, stream=side)
        side.synchronize()
        t_kernel[0] = time.perf_counter() - t0

    th = threading.Thread(target=long_batch)
    th.start()
    errors, calls = [], 0
    while th.is_alive():
        for b, w in zip(bodies, wants):
            if rpc_amd.rpc_crc32(b) != w:
                errors.append(len(b))
            calls += 1
    th.join()
    print(f"one-wave 4 GiB body: {t_kernel[0]:.2f} s, {calls} drop-in calls beside it")
    assert not errors, errors
    assert calls > 100
    host = base.cpu().numpy()
    del base
    piece = 1 << 28
    po = np.arange(0, L, piece, dtype=np.uint64)
    pl = np.minimum(np.uint64(L) - po, np.uint64(piece)).astype(np.uint32)
    parts = oracle.crc32_batch_mt(host, po, pl)
    acc = int(parts[0])
    for c, n in zip(parts[1:], pl[1:]):
        acc = oracle.combine(acc, int(c), int(n))
    assert int(u32(out)[0]) == acc


def test_drop_in_service_no_answer_falls_back():
    """VERDICT / ADVICE r04: a drop-in call whose service request gets no answer in
    time gives it up and takes the launch-per-call path (which waits on its own
    stream) instead of aborting.  Forced on the fault-injection build
    (RPCCRC_TEST_SVC_MUTE=3: the next three inline requests carry a tag that never
    matches; the first waits 20 ms); those calls and every call after them on the
    same slots must return the oracle CRC.  ADVICE r05: only the first give-up waits
    the full time -- the two after it wait the short one -- and the first answered
    call ends that state (rpc_crc32_service_stats counters, no wall-clock cutoffs)."""
    import os
    import subprocess
    import sys
    code = r"""
import json, numpy as np, rpc_amd
from oracle import oracle
bodies = [oracle.splitmix_bytes(k, 0xFA + k) for k in (68, 12, 100, 68, 1000, 68)]
for i, b in enumerate(bodies * 3):
    ok = rpc_amd.rpc_crc32(b) == oracle.crc32(b)
    print("call", i, len(b), ok)
print("stats", json.dumps(rpc_amd.service_stats()))
"""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RPCCRC_TEST_SVC_MUTE="3", PYTHONPATH=repo,
               RPCCRC_LIB=os.path.join(repo, "rpc_amd", "lib", "librpccrc_test.so"))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=180, env=env, cwd=repo)
    assert p.returncode == 0, p.stderr[-3000:]
    rows = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("call")]
    assert len(rows) == 18 and all(r[3] == "True" for r in rows), p.stdout
    import json
    st = json.loads(p.stdout.split("stats", 1)[1])
    assert st["fallbacks_full"] == 1 and st["fallbacks_short"] == 2, st
    assert st["answered"] == 15, st  # every later call through the service again
    assert st["bypassed"] == 0, st   # the instance was running all along


def test_drop_in_service_stop():
    """rpc_crc32_service_stop (a device-wide synchronize waits for the
    resident service): after a burst of drop-in calls the service leaves on request
    (rpc_crc32_service_stats: no instance running or queued), so a
    torch.cuda.synchronize() has nothing of it to wait for, and the next drop-in
    calls restart it and answer with the oracle CRC.  Stopping with no service
    running is a no-op."""
    bodies = [oracle.splitmix_bytes(k, 0x5709 + k) for k in (9, 68, 116, 117, 1024)]
    for _ in range(3):
        before = rpc_amd.service_stats()
        for b in bodies:
            assert rpc_amd.rpc_crc32(b) == oracle.crc32(b)
        st = rpc_amd.service_stats()
        assert st["answered"] - before["answered"] == len(bodies), (before, st)
        assert rpc_amd.service_stop() == 0
        st = rpc_amd.service_stats()
        assert st["running"] == 0, st
        torch.cuda.synchronize()
    assert rpc_amd.service_stop() == 0  # nothing running
    assert rpc_amd.rpc_crc32(b"123456789") == 0xCBF43926


@pytest.mark.parametrize("mb", [8, 24, 64])
def test_two_phase_stealing_grid_sizes(mb):
    """Two-phase tail stealing (round 5, crc32_rows.h rows_phase): phase 1 runs the
    static rounds up to the claiming one, phase 2 the rest with the pool protocol.
    With few workgroups (set_options max_blocks) the phase switch falls at other
    round counts and pool sizes; every CRC of uniform one-row and four-per-row
    batches and of a ragged batch must come out exact on each grid."""
    rng = np.random.default_rng(900 + mb)
    rpc_amd.set_options(max_blocks=mb)
    try:
        for n, L in ((8 * 32 * mb * 3 + 17, 256), (4 * 8 * 32 * mb * 2 + 5, 1024)):
            host = oracle.splitmix_bytes(n * L, n ^ L)
            got = u32(rpc_amd.device_uniform(to_dev(host), n, L))
            assert np.array_equal(got, oracle.crc32_uniform(host, n, L)), (n, L)
        n = 8 * 32 * mb * 2 + 9
        lens = rng.integers(0, 9000, n).astype(np.uint32)
        offs = _packed_offsets(lens, 3)
        host = oracle.splitmix_bytes(int(lens.sum()) + 32, 901 + mb)
        _ragged_check(host, offs, lens)
    finally:
        rpc_amd.set_options(max_blocks=0)
