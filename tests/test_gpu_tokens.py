"""The Sender's channel bytes framed on the GPU from a source in HBM (token_frame_kernel; rsh_tokens_write_device,
rsh_tokens_write_kept, rsh_tokens_write_batch_device) against the host writer rsh_tokens_write and the oracle's
orc_tokens, byte for byte.  Every host output buffer has 64 guard bytes of 0xA5 on each side, checked after every
call (the binding's tokens_* methods do it and raise; the JNI test does it here)."""
import ctypes
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

import oracle_ctypes as O
import rsync_hip as R
import tokens_cases as TC
from conftest import ROOT, golden

pytestmark = pytest.mark.gpu
SEED = bytes([1, 2, 3, 4])
SEED_NP = np.frombuffer(SEED, np.uint8).copy()


@pytest.fixture(scope="module")
def ctx():
    R.build()
    c = R.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def crafted(ctx):
    """The crafted stream's source in a device buffer of exactly N bytes (a literal ends at its last byte), the
    events and the host writer's bytes: computed once, read by every test."""
    src, ev = TC.source(), TC.crafted()
    d = ctx.alloc(TC.N)
    d.upload(src)
    yield d, ev, R.tokens(src, ev, TC.MD5)
    d.free()


# ---- 1. crafted streams ----

def test_crafted_events_cover_the_cases(crafted):
    _, ev, ref = crafted
    lits = [e for e in ev if e["kind"] == R.EV_LITERAL]
    runs = [e for e in ev if e["kind"] == R.EV_MATCH]
    assert {int(e["length"]) for e in lits} >= set(TC.LIT_LENGTHS)
    assert {int(e["offset"]) % 16 for e in lits} >= set(TC.SRC_RESIDUES)
    assert any(int(e["offset"]) + int(e["length"]) == TC.N for e in lits)
    assert {int(e["count"]) for e in runs} >= {1, 2, 5, 4099}
    assert {int(e["index"]) for e in runs} >= {0, 2**31 - 4200}
    assert {o % 16 for o in TC.offsets(ev)[:-1]} == set(range(16))
    assert len(ref) == R.tokens_size(ev)


@pytest.mark.parametrize("span,piece", [(None, None), (64, 8 << 10), (4096, 8 << 10), (8196, None)],
                         ids=["default", "span64", "span4096", "span8196"])
def test_crafted_stream(ctx, crafted, rsh_opt, span, piece):
    d, ev, ref = crafted
    if span:
        rsh_opt("tokens_span", span)
    if piece:
        rsh_opt("tokens_piece", piece)
    assert ctx.tokens_device(d, TC.N, ev, TC.MD5) == ref


@pytest.mark.parametrize("span", [None, 1 << 20, 100000])
def test_long_literal_over_several_workgroups(ctx, rsh_opt, span):
    """A span longer than the 64 KiB a workgroup frames (the kernel cuts it over blockIdx.y): one literal of 400 KiB
    less 3 bytes at an odd source offset, a match run before it so that the destination phase is odd too, whole and
    through windows that start inside it."""
    if span:
        rsh_opt("tokens_span", span)
    n = 400 << 10
    src = O.splitmix(n, 0x10A6)
    ev = np.zeros(2, R.EVENT_DTYPE)
    ev[0] = (0, 0, R.EV_MATCH, 11, 3, 0)
    ev[1] = (3, n - 3, R.EV_LITERAL, 0, 0, 0)
    d = ctx.alloc(n)
    d.upload(src)
    ref = R.tokens(src, ev, TC.MD5)
    assert ctx.tokens_device(d, n, ev, TC.MD5) == ref
    for start, length in ((65536 + 7, 200001), (12 + 8196 * 9 + 2, 70000), (131072, len(ref) - 131072)):
        assert ctx.tokens_device(d, n, ev, TC.MD5, start, length) == ref[start:start + length], (start, length)
    d.free()


def test_empty_list_is_the_trailer(ctx):
    none = np.zeros(0, R.EVENT_DTYPE)
    assert ctx.tokens_device(None, 0, none, TC.MD5) == bytes(4) + TC.MD5
    assert ctx.tokens_device(None, 0, none, TC.MD5, 3, 5) == (bytes(4) + TC.MD5)[3:8]
    assert ctx.tokens_device(None, 0, none, TC.MD5, 20, 0) == b""


def test_matches_need_no_source(ctx, crafted):
    _, ev, _ = crafted
    runs = ev[ev["kind"] == R.EV_MATCH]
    assert ctx.tokens_device(None, 0, runs, TC.MD5) == R.tokens(b"", runs, TC.MD5)


def test_bad_arguments_launch_nothing(ctx, crafted):
    d, ev, ref = crafted
    bad = ev.copy()
    bad[0]["length"] = TC.N + 1
    with pytest.raises(ValueError):
        ctx.tokens_device(d, TC.N, bad, TC.MD5)
    with pytest.raises(ValueError):
        ctx.tokens_device(d, TC.N - 1, ev, TC.MD5)      # the literal that ends at N reaches past N - 1
    with pytest.raises(ValueError):
        ctx.tokens_device(None, TC.N, ev, TC.MD5)       # literals without a source
    for start, length in ((-1, 1), (0, -1), (len(ref), 1), (1, len(ref))):
        with pytest.raises(ValueError):
            ctx.tokens_device(d, TC.N, ev, TC.MD5, start, length)


# ---- 2. windows ----

@pytest.mark.parametrize("span,piece", [(None, None), (64, 8 << 10), (4096, 8 << 10)],
                         ids=["default", "span64", "span4096"])
def test_windows(ctx, crafted, rsh_opt, span, piece):
    d, ev, ref = crafted
    if span:
        rsh_opt("tokens_span", span)
        rsh_opt("tokens_piece", piece)
    for start, length in TC.windows(ev):
        assert ctx.tokens_device(d, TC.N, ev, TC.MD5, start, length) == ref[start:start + length], (start, length)


def test_consecutive_windows_concatenate(ctx, crafted):
    d, ev, ref = crafted
    parts = [ctx.tokens_device(d, TC.N, ev, TC.MD5, s, min(4099, len(ref) - s)) for s in range(0, len(ref), 4099)]
    assert b"".join(parts) == ref


# ---- 3. scans end to end ----

WITH_BASIS = [c for c in golden() if c["basis"] is not None]


def _oracle_stream(case, h=None):
    oh = O.Header(**case["header"]) if h is None else h
    weak = np.array(case["weak"], np.int32) if h is None else np.zeros(0, np.int32)
    strong = np.frombuffer(bytes.fromhex(case["strong"]), np.uint8).copy() if h is None else np.zeros(0, np.uint8)
    oev, ofm, _, _, _ = O.sender(case["src_bytes"], oh, weak, strong, case["seed_bytes"])
    return weak, strong, O.tokens(case["src_bytes"], oev, ofm)


@pytest.mark.parametrize("case", WITH_BASIS, ids=lambda c: c["name"])
def test_scan_then_kept_tokens_match_oracle(ctx, case):
    weak, strong, want = _oracle_stream(case)
    rh = R.Header(**case["header"])
    ev, fm, _, _, _ = ctx.match_scan(case["src_bytes"], rh, weak, strong, case["seed_bytes"])
    got = ctx.tokens_kept(ev, fm)
    assert got == want
    assert hashlib.sha256(got).hexdigest() == case["tokens_sha256"]
    target, res = ctx.receiver_combine(got, rh, case["basis_bytes"])
    assert target == case["src_bytes"] and res.tokens_used == len(got) - 16 and bytes(res.md5) == fm


@pytest.mark.parametrize("name", ["identical_20480", "insert_100", "new_file"])
def test_file_scan_then_kept_tokens(ctx, tmp_path, name):
    cases = {c["name"]: c for c in WITH_BASIS}
    new = name == "new_file"
    case = cases["half_modified" if new else name]
    p = tmp_path / "src.bin"
    p.write_bytes(case["src_bytes"])
    if new:  # Sender.skipMatchSendData: block_length 0, no table
        _, _, want = _oracle_stream(case, O.header(0, 0, 0))
        rh, weak, strong = R.Header(0, 0, 0, 0), np.zeros(0, np.int32), np.zeros(0, np.uint8)
    else:
        weak, strong, want = _oracle_stream(case)
        rh = R.Header(**case["header"])
    ev, fm, _, _, _, err = ctx.match_scan_file(str(p), len(case["src_bytes"]), rh, weak, strong, case["seed_bytes"])
    assert not err
    got = ctx.tokens_kept(ev, fm)
    assert got == want
    target, _ = ctx.receiver_combine(got, rh, None if new else case["basis_bytes"])
    assert target == case["src_bytes"]


# ---- 4. the kept source's lifetime ----

def test_kept_source_lifetime(tmp_path, rsh_opt):
    case = {c["name"]: c for c in WITH_BASIS}["insert_100"]
    weak, strong, want = _oracle_stream(case)
    rh = R.Header(**case["header"])
    src, seed = case["src_bytes"], case["seed_bytes"]
    p = tmp_path / "src.bin"
    p.write_bytes(src)
    with R.Context(0) as c:
        none = np.zeros(0, R.EVENT_DTYPE)
        with pytest.raises(R.NoSourceError):      # a fresh context
            c.tokens_kept(none, TC.MD5)

        def scan():
            ev, fm, _, _, _ = c.match_scan(src, rh, weak, strong, seed)
            return ev, fm

        ev, fm = scan()
        assert c.tokens_kept(ev, fm) == want
        assert c.tokens_kept(ev, fm, 5, 100) == want[5:105]   # a tokens call keeps the record
        c.block_sums(case["basis_bytes"], rh, seed)             # reuses the staging the source was in
        with pytest.raises(R.NoSourceError):
            c.tokens_kept(ev, fm)
        ev, fm = scan()
        assert c.tokens_kept(ev, fm) == want                  # works again after the next resident scan
        c.trim()
        with pytest.raises(R.NoSourceError):
            c.tokens_kept(ev, fm)
        ev, fm = scan()
        assert c.tokens_kept(ev, fm) == want
        rsh_opt("file_tile_above", 1 << 12)                    # the file scan goes tiled: HBM holds one tile
        rsh_opt("file_tile", 1 << 13)
        ev2, fm2, _, _, _, _ = c.match_scan_file(str(p), len(src), rh, weak, strong, seed)
        assert fm2 == fm and R.events_as_tuples(ev2, rh.block_length) == R.events_as_tuples(ev, rh.block_length)
        with pytest.raises(R.NoSourceError):
            c.tokens_kept(ev2, fm2)
        R.reset_options()
        ev3, fm3, _, _, _, _ = c.match_scan_file(str(p), len(src), rh, weak, strong, seed)
        assert c.tokens_kept(ev3, fm3) == want


# ---- 5. a segment ----

def _segment(rng, count):
    """Mixed shapes, as test_gpu_batch.py's segment: block lengths that take the coalesced and the per-lane K1, files
    shorter than a block, identical / every-other-block / mutated sources."""
    from test_resolver_cpu import _mutate
    files = []
    for i in range(count):
        B = rng.choice([512, 640, 700, 1024, 2048, 8192, 8192])
        kind = rng.random()
        nb = rng.randrange(1, B) if kind < 0.1 else 64 * B if kind < 0.2 else rng.randrange(B, 60 * B)
        key = rng.randrange(1 << 62)
        basis = O.splitmix(nb, key).tobytes()
        r = rng.random()
        if r < 0.15:
            src = basis
        elif r < 0.3:
            other = O.splitmix(nb, key ^ 0xED17).tobytes()
            src = b"".join(other[k:k + B] if (k // B) % 2 else basis[k:k + B] for k in range(0, nb, B))
        else:
            src = _mutate(rng, basis, B, key) or basis
        files.append((basis, src, B, rng.choice([2, 3, 4, 16])))
    return files


def _pack(ctx, blobs, misalign):
    offs, pos = [], 0
    for b, m in zip(blobs, misalign):
        pos = (pos + 255) // 256 * 256 + m
        offs.append(pos)
        pos += max(len(b), 1)
    host = np.zeros(pos + 1, np.uint8)
    for b, o in zip(blobs, offs):
        host[o:o + len(b)] = np.frombuffer(b, np.uint8)
    d = ctx.alloc(host.size)
    d.upload(host)
    return d, offs


def test_segment_tokens(ctx, rsh_opt):
    rsh_opt("tokens_piece", 256 << 10)  # several staging passes, files straddling them
    rng = random.Random(4040)
    files = _segment(rng, 40)
    mis = [0 if rng.random() < 0.6 else rng.choice([1, 3, 4, 8, 15]) for _ in files]
    d_src, soffs = _pack(ctx, [f[1] for f in files], mis)
    heads = [R.header_make(B, dl, len(basis)) for basis, _, B, dl in files]
    tables = [O.generator(basis, O.header(B, dl, len(basis)), SEED) for basis, _, B, dl in files]
    d_tabs = []
    sj = (R.ScanJob * len(files))()
    evs = []
    for i, (h, (basis, src, B, dl)) in enumerate(zip(heads, files)):
        w, s = tables[i]
        dw, ds = ctx.alloc(4 * h.chunk_count + 4), ctx.alloc(h.chunk_count * dl + 1)
        dw.upload(w)
        ds.upload(s)
        d_tabs.append((dw, ds))
        cap = len(src) // (10 * B) + 2 * h.chunk_count + 64
        ev = np.zeros(cap, R.EVENT_DTYPE)
        evs.append(ev)
        sj[i].d_src, sj[i].n, sj[i].h = d_src.ptr.value + soffs[i], len(src), h
        sj[i].d_weak, sj[i].d_strong = dw.ptr.value, ds.ptr.value
        sj[i].ev, sj[i].ev_cap = ev.ctypes.data, cap
    assert R.lib().rsh_match_scan_batch_device(ctx.handle, sj, len(files), SEED_NP.ctypes.data, None) == 0
    evs = [ev[:sj[i].n_ev].copy() for i, ev in enumerate(evs)]
    md5s = [hashlib.md5(f[1]).digest() for f in files]
    want = [R.tokens(f[1], ev, m) for f, ev, m in zip(files, evs, md5s)]

    jobs = [(d_src.ptr.value + soffs[i], len(files[i][1]), evs[i], md5s[i]) for i in range(len(files))]
    rc, res = ctx.tokens_batch_device(jobs)
    assert rc == R.RSH_OK
    for i, (st, got, out_len) in enumerate(res):
        assert st == R.RSH_OK and got == want[i] and out_len == len(want[i]), i

    # one file's buffer a byte short, one file's literal reaching past its source: only those two fail
    short = 7
    past = next(i for i, ev in enumerate(evs) if i != short and (ev["kind"] == R.EV_LITERAL).any())
    bad = evs[past].copy()
    k = int(np.nonzero(bad["kind"] == R.EV_LITERAL)[0][-1])
    bad[k]["length"] = len(files[past][1]) - int(bad[k]["offset"]) + 1
    jobs[short] = jobs[short] + (len(want[short]) - 1,)
    jobs[past] = (jobs[past][0], jobs[past][1], bad, jobs[past][3])
    rc, res = ctx.tokens_batch_device(jobs)
    assert rc == (R.RSH_E_NOSPACE if short < past else R.RSH_E_INVAL)
    for i, (st, got, out_len) in enumerate(res):
        if i == short:
            assert st == R.RSH_E_NOSPACE and out_len == len(want[i])
        elif i == past:
            assert st == R.RSH_E_INVAL
        else:
            assert st == R.RSH_OK and got == want[i], i
    for dw, ds in d_tabs:
        dw.free()
        ds.free()
    d_src.free()


# ---- 6. through the staging at size ----

def test_new_file_64mib_whole_and_windows(ctx, tmp_path):
    n = 64 << 20
    src = O.splitmix(n, 0x64AB)
    p = tmp_path / "big.bin"
    src.tofile(str(p))
    ev, fm, lit, _, _, err = ctx.match_scan_file(str(p), n, R.Header(0, 0, 0, 0), np.zeros(0, np.int32),
                                                 np.zeros(0, np.uint8), SEED)
    assert not err and lit == n and fm == hashlib.md5(src.tobytes()).digest()
    want = hashlib.sha256(R.tokens(src, ev, fm)).hexdigest()
    size = R.tokens_size(ev)
    assert hashlib.sha256(ctx.tokens_kept(ev, fm)).hexdigest() == want
    acc = hashlib.sha256()
    win = (5 << 20) + 1
    for start in range(0, size, win):
        acc.update(ctx.tokens_kept(ev, fm, start, min(win, size - start)))
    assert acc.hexdigest() == want


# ---- 7. the JNI shim ----

def test_jni_tokens_kept():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "java-rsync_amd"), "jni-harness"], check=True)
    H = ctypes.CDLL(os.path.join(ROOT, "java-rsync_amd", "lib", "libjniharness.so"))
    H.jh_exception.restype = ctypes.c_char_p
    H.jh_ctx_create.restype = ctypes.c_int64
    H.jh_match_scan.restype = ctypes.c_int64
    case = {c["name"]: c for c in WITH_BASIS}["half_modified"]
    weak, strong, want = _oracle_stream(case)
    h = case["header"]
    hdr = np.array([h["chunk_count"], h["block_length"], h["digest_length"], h["remainder"]], np.int32)
    src = np.frombuffer(case["src_bytes"], np.uint8).copy()
    seed = np.frombuffer(case["seed_bytes"], np.uint8).copy()
    md5, sizes, quads = np.zeros(16, np.uint8), np.zeros(2, np.int64), np.zeros(4 * 4096, np.int64)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    i64 = ctypes.c_int64
    c = H.jh_ctx_create(0)
    assert c != 0 and H.jh_exception() == b""
    try:
        k = H.jh_match_scan(i64(c), p(src), i64(src.size), i64(src.size), p(hdr), p(weak), i64(weak.size), p(strong),
                            i64(strong.size), p(seed), i64(4), p(md5), i64(16), p(sizes), i64(2), p(quads),
                            i64(quads.size))
        assert H.jh_exception() == b"" and 0 < k <= quads.size and k % 4 == 0
        whole = np.full(len(want) + 128, 0xA5, np.uint8)
        out = whole[64:64 + len(want)]

        def kept(start, length):
            return H.jh_tokens_kept(i64(c), p(quads), i64(k), k // 4, p(md5), i64(16), i64(start), p(out[start:]),
                                    i64(length), i64(length))

        assert kept(0, len(want)) == 1 and H.jh_exception() == b""
        assert out.tobytes() == want and (whole[:64] == 0xA5).all() and (whole[-64:] == 0xA5).all()
        out[:] = 0
        assert kept(9, 1000) == 1 and out[9:1009].tobytes() == want[9:1009] and not out[:9].any() and not out[1009:].any()
        H.jh_ctx_trim(i64(c))
        assert H.jh_exception() == b""
        assert kept(0, len(want)) == 0 and H.jh_exception() == b""   # no source: false, not an exception
    finally:
        H.jh_ctx_destroy(i64(c))
