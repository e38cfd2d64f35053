"""The byte movers' case tables (tests/io_cases.py) without a device: the closed-form weak sum against the oracle's
Generator, every class a classifier names reached by some case, the tables' sizes, and the classifiers' constants read
back from device_io.hip."""
import os

import numpy as np

import io_cases as IO
import oracle_ctypes as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = bytes([1, 2, 3, 4])


def _classes(T, D):
    return [IO.gather_class(op.sphase, op.dphase, op.length, T, D) for op in IO.gather_table(T, D)]


def test_table_sizes_are_pinned():
    assert len(IO.gather_table(256, 2)) == 768 + 237 + 27
    assert len(IO.gather_table(1024, 4)) == 768 + 285 + 27
    assert len(IO.COPY_FEW) == 60 + 15 and len(IO.COPY_MANY) == 48 and len(IO.COPY_TO_HOST) == 20
    assert len(IO.window_shapes()) == 3 * 60 + 15 and len(IO.WINDOWS) == 2340 == len(set(IO.WINDOWS))
    assert len(IO.window_launches()) == 852 and sum(len(l[4]) for l in IO.window_launches()) == 2340
    assert len(IO.BLOCK_FILES) == 9
    for T, D in IO.GATHER_FORMS:
        ops = IO.gather_table(T, D)
        assert all(op.length > 0 for op in ops)
        assert max(op.length for op in ops) == 2 * D * 16 * T + 16 + 30
        # the whole table's device footprint, sources and destinations with their guards: far below 256 MiB
        assert 2 * sum(op.length + IO.GUARD + 32 for op in ops) < 256 << 20


def test_constants_are_the_kernels():
    """A change of a launcher's shape in device_io.hip fails here instead of silently moving the tables' edges."""
    text = open(os.path.join(ROOT, "java-rsync_amd", "csrc", "device_io.hip")).read()
    c = IO.source_constants(text)
    assert c["forms"] == IO.GATHER_FORMS == [(256, 2), (1024, 4)]
    assert c["switch"] == IO.GATHER_SWITCH == 64 << 10
    assert c["few"] == c["many"] == (IO.COPY_WG_BYTES, IO.COPY_MAX_WGS, IO.COPY_THREADS) == (4096, 64, 256)
    assert c["window_threads"] == IO.WINDOW_THREADS == 256
    assert IO.gather_form(0) == IO.gather_form((64 << 10) - 1) == (256, 2)
    assert IO.gather_form(64 << 10) == IO.gather_form(1 << 20) == (1024, 4)


def test_gather_class_follows_the_issue_sketch():
    """The classifier at hand-worked ranges of the 1024 / 4 form (step 16384)."""
    g = IO.gather_class(3, 15, 1 + 4 * 16384 + 16 + 15, 1024, 4)  # head 1, then src % 16 = 4
    assert (g["head"], g["cls"], g["unrolled0"], g["body"], g["tail"]) == (1, "word", 0, 65552, 15)
    g = IO.gather_class(0, 0, 3 * 16384 + 16, 1024, 4)
    assert (g["cls"], g["unrolled0"], g["unrolled_threads"], g["single"]) == ("x4", 1, 1, True)
    g = IO.gather_class(0, 0, 3 * 16384, 1024, 4)
    assert (g["unrolled0"], g["unrolled_threads"], g["single"]) == (0, 0, True)
    g = IO.gather_class(1, 1, 15 + 4 * 16384, 1024, 4)
    assert (g["head"], g["cls"], g["unrolled0"], g["unrolled_threads"], g["single"]) == (15, "x4", 1, 1024, False)
    g = IO.gather_class(0, 0, 7 * 16384 + 16, 1024, 4)
    assert (g["unrolled0"], g["unrolled_threads"]) == (2, 1024)
    g = IO.gather_class(9, 14, 1, 256, 2)
    assert g["head_only"] and (g["head"], g["body"], g["tail"]) == (1, 0, 0)


def test_gather_tables_reach_every_class():
    for T, D in IO.GATHER_FORMS:
        cl = _classes(T, D)
        ops = IO.gather_table(T, D)
        assert {(op.dphase, op.sphase) for op in ops} == {(d, s) for d in range(16) for s in range(16)}
        for cls in ("x4", "word", "byte"):
            for headed in (False, True):
                for body_kind in (0, 1):  # with and without a body
                    assert any(c["cls"] == cls and (c["head"] > 0) == headed and (c["body"] > 0) == bool(body_kind)
                               and not c["head_only"] for c in cl), (T, D, cls, headed, body_kind)
                assert {c["tail"] for c in cl if c["cls"] == cls and (c["head"] > 0) == headed
                        and c["body"] > 16 * T} >= {0, 1, 15}, (T, D, cls, headed)
        x4 = [c for c in cl if c["cls"] == "x4"]
        assert {c["unrolled0"] for c in x4} == {0, 1, 2}
        assert {c["unrolled0"] for c in x4 if c["head"] > 0} == {0, 1, 2}
        counts = {c["unrolled_threads"] for c in x4}
        assert 0 in counts and T in counts and any(0 < k < T for k in counts), "no / every / some threads unrolled"
        assert any(c["unrolled0"] == 2 and c["unrolled_threads"] == T for c in x4)
        assert {c["single"] for c in x4 if c["unrolled0"] > 0} == {False, True}
        # the bodies of the issue, each with every tail, in every class
        for cls in ("x4", "word", "byte"):
            assert {(c["body"], c["tail"]) for c in cl if c["cls"] == cls} >= \
                {(b, t) for b in IO.bodies(T, D) for t in IO.TAILS if b + t > 0}, (T, D, cls)
        ho = [(op, c) for op, c in zip(ops, cl) if c["head_only"]]
        assert {c["head"] for _, c in ho} >= {1, 14} and all(1 <= op.length < IO.head_of(op.dphase) for op, _ in ho)
        assert {IO.head_of(op.dphase) for op, _ in ho} == set(range(2, 16))
        assert all(c["head"] + c["body"] + c["tail"] == op.length for op, c in zip(ops, cl))


def test_copy_tables_reach_every_class():
    few = [(op, IO.copy_class(op, "few", max(o.length for o in launch))) for launch in IO.COPY_FEW for op in launch]
    for cls in ("x4", "piece"):
        for headed in (False, True):
            got = {op.length for op, c in few if c["cls"] == cls and (c["head"] > 0) == headed}
            # (a range no longer than its head has no pieces: its class is only a name)
            assert got >= {n for n in IO.COPY_LENGTHS if n > 15}, (cls, headed)
    assert {op.length for op, c in few if c["head"] == op.length} >= {1, 15}
    assert {op.length for op, c in few if c["head"] == 0} >= {1, 15}
    assert {c["wgs"] for _, c in few} >= {1, 2, 64} and max(c["strides"] for _, c in few) >= 2
    assert any(c["strides"] == 1 and c["wgs"] == 64 for _, c in few)  # 262144: the last size without a stride
    assert {len(launch) for launch in IO.COPY_FEW} == {1, 2, 3, 4}
    for launch in IO.COPY_FEW:
        if len(launch) > 1:
            lens = [op.length for op in launch]
            assert len(set(lens)) == len(lens) and min(lens) * 16 <= max(lens)
    # a short range in every slot before and after the one that sizes the grid
    assert {launch.index(max(launch, key=lambda o: o.length)) for launch in IO.COPY_FEW if len(launch) > 1} >= {0, 1, 2, 3}
    for form in ("many", "bg"):
        cl = [IO.copy_class(op, form, max(IO.COPY_LENGTHS)) for op in IO.COPY_MANY]
        assert {c["wgs"] for c in cl} == {64 if form == "many" else 1}
        assert {op.sphase for op in IO.COPY_MANY} == set(IO.COPY_SRC_PHASES)
        assert max(c["strides"] for c in cl) == (3 if form == "many" else -(-524293 // 16 // 256))
        assert {c["last"] for c in cl} >= {0, 1, 15}
    assert {(op.length, op.sphase) for op in IO.COPY_TO_HOST} == {(n, s) for n in (1, 15, 16, 17, 4096 * 3 + 5)
                                                                   for s in IO.COPY_SRC_PHASES}
    assert {IO.copy_class(op, "host")["wgs"] for op in IO.COPY_TO_HOST} == {1, 4}


def test_window_table_reaches_every_class():
    cl = [IO.window_class(c.p, min(c.B, c.n - c.p)) for c in IO.WINDOWS]
    full = [k for c, k in zip(IO.WINDOWS, cl) if c.B <= c.n - c.p]
    assert {(k["head"], k["R"], k["tail"]) for k in full} >= \
        {(h, R, t) for h in IO.WINDOW_HEADS for R in IO.WINDOW_R for t in IO.TAILS if h + R + t > 0}
    assert {k["unrolled0"] for k in full} == {0, 1, 2}
    counts = {k["unrolled_threads"] for k in full}
    assert counts >= {0, 1, 256}, "no thread, thread 0 alone (some but not all) and every thread in the eight-load loop"
    assert {k["last_piece"] for k in full} >= {0, 16, 48}
    assert IO.window_class(0, 16448)["unrolled_threads"] == 1 and IO.window_class(0, 16447)["unrolled_threads"] == 0
    assert IO.window_class(0, 49216)["unrolled0"] == 2 and IO.window_class(0, 49215)["unrolled0"] == 1
    short = [(c, k) for c, k in zip(IO.WINDOWS, cl) if c.B > c.n - c.p]
    assert {c.n - c.p for c, _ in short} == {1, 15, 16, 17, IO.SHORT_B - 1}
    assert {k["head"] for _, k in short} == {0, 1, 15}
    assert any(k["head"] == c.n - c.p == 1 and k["R"] == 0 for c, k in short)  # the head clipped to the window
    for sel in (full, [k for _, k in short]):
        assert {k["head"] for k in sel} >= {0, 1, 15} and {k["tail"] for k in sel} >= {0, 1, 15}
    assert {(c.base, c.pattern) for c in IO.WINDOWS} == {(b, p) for b in IO.WINDOW_BASES for p in IO.PATTERNS}
    assert all(c.n <= IO.FILE_BYTES and c.p + min(c.B, c.n - c.p) <= c.n for c in IO.WINDOWS)
    assert {(f.B, f.n - 5 * f.B) for f in IO.BLOCK_FILES} == {(B, r) for B in IO.BLOCK_BS for r in (0, 1, B - 1)}
    assert {f.base for f in IO.BLOCK_FILES} == set(IO.WINDOW_BASES) and {f.pattern for f in IO.BLOCK_FILES} == set(IO.PATTERNS)


def test_closed_form_weak_sum_is_the_generators():
    """weak_sum against O.generator's weak sum of the same window taken as a one-chunk file: every pattern, every head
    and tail, the shortest and the longest window."""
    longest = max(min(c.B, c.n - c.p) for c in IO.WINDOWS)
    sample = [c for c in IO.WINDOWS if c.base == 0 and
              (min(c.B, c.n - c.p) in (1, 16, 17, 49, IO.SHORT_B - 1, 16384, 16479, longest))]
    assert {c.pattern for c in sample} == set(IO.PATTERNS) and len(sample) >= 40
    assert any(min(c.B, c.n - c.p) == longest for c in sample) and longest == 15 + 49232 + 15
    for c in sample:
        w = min(c.B, c.n - c.p)
        x = np.ascontiguousarray(IO.window_file(c.pattern)[c.p:c.p + w])
        weak, _ = O.generator(x, O.header(w, 2, w), SEED)
        assert weak.size == 1 and int(weak[0]) == IO.window_want(c), IO.window_id(c)
    # the signs: all 0x80 is -128 per byte, all 0x7f is 127; S2 wraps 16 bits long before the longest window ends
    assert IO.weak_sum(np.full(3, 0x80, np.uint8)) == ((-384) & 0xFFFF | ((-768) & 0xFFFF) << 16) - (1 << 32)
    assert IO.weak_sum(np.full(2, 0x7F, np.uint8)) == 254 | 381 << 16


def test_pack_places_ranges_between_guards():
    ops = IO.gather_table(256, 2)[:60] + IO.gather_table(256, 2)[-27:]
    edge = [3, 40, len(ops) - 1]
    P = IO.pack(ops, 77, edge=edge)
    assert P.edge_src.size == P.src_off[edge[-1]] + ops[edge[-1]].length  # the last edge source ends its buffer
    spans = []
    for i, op in enumerate(ops):
        buf = P.edge_src if i in P.edge_ops else P.src
        assert P.src_off[i] % 16 == op.sphase and P.dst_off[i] % 16 == op.dphase
        assert P.src_off[i] + op.length <= buf.size - (0 if i in P.edge_ops else IO.SLACK)
        assert np.array_equal(buf[P.src_off[i]:P.src_off[i] + op.length], P.image[P.dst_off[i]:P.dst_off[i] + op.length])
        spans.append((P.dst_off[i], P.dst_off[i] + op.length))
    assert spans[0][0] >= IO.GUARD and P.dst_size - spans[-1][1] >= IO.GUARD
    assert all(b[0] - a[1] >= IO.GUARD for a, b in zip(spans, spans[1:]))
    outside = np.ones(P.dst_size, bool)
    for a, b in spans:
        outside[a:b] = False
    assert (P.image[outside] == IO.FILL).all()
    got = P.image.copy()
    assert IO.mismatches(P, got) == ([], True)
    got[spans[5][1] + 3] ^= 1  # a byte of the guard after range 5
    got[spans[9][0]] ^= 1
    assert IO.mismatches(P, got) == ([5, 9], True)
    assert IO.shuffled(10, 3) == IO.shuffled(10, 3) != list(range(10)) and sorted(IO.shuffled(10, 3)) == list(range(10))
