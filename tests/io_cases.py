"""Shared case tables of the byte movers' lattice (tests/test_io_cases_cpu.py, tests/test_gpu_io_lattice.py): the
ranges gather_ops_kernel_t, copy_few_kernel, copy_many_kernel and copy_to_host_kernel move and the windows
window_weak_kernel sums over range_sums (device_io.hip, device_common.h), classifiers that restate which branch and
which loop edge a case takes, a closed form of the weak sum and a packer that lays a table's ranges out in one source
and one destination buffer with guard bytes.  Plain module: no device.

What the classifiers restate, with the code they follow:
  gather_class  gather_ops_kernel_t<T, D>: the byte-wise head up to the destination's 16-byte boundary, the body by the
                source's alignment after it (x4: 16-byte loads, D of them in flight in the unrolled loop, then single
                steps; word: four dword loads; byte: sixteen byte loads), the byte-wise tail
  copy_class    copy_few_kernel (the same head, then 16-byte loads or copy_piece by the source's alignment, 4096 bytes
                per workgroup and a grid stride past 64 workgroups), copy_many_kernel (copy_piece alone; one workgroup
                per range in the background form) and copy_to_host_kernel (copy_piece, no stride)
  window_class  range_sums at 256 threads: the byte head up to the position's 16-byte boundary, the eight-load loop,
                the loop of 64-byte pieces with its short last piece, the byte tail

The tables:
  gather_table(T, D)  every (dst phase, src phase) of the 16 x 16 grid at the bodies 0, step + 16 and D step + 16 (tails
                      1 and 15 in turn) -- 768; every body of bodies(T, D) x the tails 0, 1, 15 at the phase pairs of
                      PHASES, without the three empty ranges -- 285 at D = 4, 237 at D = 2; the head-only ranges -- 27
  COPY_FEW            launches of one range (COPY_LENGTHS x COPY_PHASES) and of two to four ranges of unequal length
  COPY_MANY           COPY_LENGTHS x COPY_SRC_PHASES in one launch, at high priority and in the background form
  COPY_TO_HOST        HOST_LENGTHS x COPY_SRC_PHASES, a launch each
  WINDOWS             WINDOW_R x heads 0, 1, 15 x tails 0, 1, 15 as full windows (w = B: 60 block lengths at three
                      positions each) and the short windows of SHORT_B, each at the bases WINDOW_BASES and in the
                      patterns PATTERNS -- 2340, in 852 launches
  BLOCK_FILES         the aligned windows of files of 5 B + r bytes, the by_block form -- 9"""
import random
import re
from collections import namedtuple

import numpy as np

import oracle_ctypes as O

GATHER_FORMS = [(256, 2), (1024, 4)]  # (T, D) of launch_gather_ops' two instantiations
GATHER_SWITCH = 64 << 10              # avg_len below it: the 256-thread form
COPY_WG_BYTES, COPY_MAX_WGS, COPY_THREADS = 4096, 64, 256  # launch_copy_few / launch_copy_many
WINDOW_THREADS = 256
GUARD = 64    # bytes between two packed destinations, at least
FILL = 0xA5   # what a destination buffer holds before a launch
SLACK = 256   # bytes after the last source inside the main source buffer (tests/test_gpu_k1_shapes.py)

TAILS = [0, 1, 15]
PHASES = [(0, 0), (1, 1), (1, 0), (8, 4), (15, 3), (4, 15), (0, 1), (0, 4)]  # (dst, src): every source class, with and without a head

Op = namedtuple("Op", "dphase sphase length")


def head_of(dphase, length=1 << 62):
    return min(length, (16 - dphase % 16) % 16)


def bodies(T, D):
    """The body lengths (multiples of 16) around the loops' edges: no unrolled iteration, thread 0 only, every thread,
    a second iteration for thread 0."""
    step = 16 * T
    return sorted({0, 16, step - 16, step, step + 16, (D - 1) * step, (D - 1) * step + 16, D * step - 16, D * step,
                   D * step + 16, (2 * D - 1) * step + 16, 2 * D * step + 16})


def gather_class(src, dst, length, T, D):
    """The path gather_ops_kernel_t<T, D> takes over a range (src, dst: addresses or phases): head bytes, source class
    after the head, thread 0's unrolled iterations, how many threads take one, whether the single-step loop runs for
    some thread, the body and the tail."""
    step = 16 * T
    head = min(length, (16 - dst % 16) % 16)
    body = (length - head) & ~15
    s = (src + head) % 16
    cls = "x4" if s == 0 else "word" if s % 4 == 0 else "byte"
    first = (D - 1) * step  # thread t enters the unrolled loop when 16 t + first < body
    it0 = 0 if body <= first else -(-(body - first) // (D * step))
    threads = 0 if body <= first else min(T, -(-(body - first) // 16))
    single = False  # some thread's k after its unrolled iterations is still below body
    if cls == "x4":
        k = 16 * np.arange(T, dtype=np.int64)
        k += np.where(k + first < body, -(-(body - first - k) // (D * step)), 0) * (D * step)
        single = bool((k < body).any())
    return dict(head=head, cls=cls, unrolled0=it0 if cls == "x4" else 0,
                unrolled_threads=threads if cls == "x4" else 0, single=single, body=body, tail=length - head - body,
                head_only=length < (16 - dst % 16) % 16)


def gather_form(avg_len):
    """(T, D) of the instantiation launch_gather_ops takes."""
    return GATHER_FORMS[0] if avg_len < GATHER_SWITCH else GATHER_FORMS[1]


_GATHER = {}


def gather_table(T, D):
    if (T, D) not in _GATHER:
        step, out = 16 * T, []
        for d in range(16):
            for s in range(16):
                for k, body in enumerate((0, step + 16, D * step + 16)):
                    out.append(Op(d, s, head_of(d) + body + (1, 15)[(d + s + k) % 2]))
        for d, s in PHASES:
            for body in bodies(T, D):
                for tail in TAILS:
                    if head_of(d) + body + tail > 0:
                        out.append(Op(d, s, head_of(d) + body + tail))
        for d in range(1, 15):  # head-only: the range ends before the destination's 16-byte boundary
            for length in sorted({1, head_of(d) - 1}):
                out.append(Op(d, (5 * d + 3) % 16, length))
        _GATHER[(T, D)] = out
    return _GATHER[(T, D)]


# ---- the copies ----

COPY_LENGTHS = [0, 1, 15, 16, 17, 4095, 4096, 4097, 262143, 262144, 262161, 524293]
COPY_PHASES = [(0, 0), (1, 1), (0, 1), (3, 8), (15, 0)]  # copy_few: 16-byte loads / copy_piece, without and with a head
COPY_SRC_PHASES = [0, 1, 4, 15]                           # copy_many: the destinations stay 16-byte aligned
HOST_LENGTHS = [1, 15, 16, 17, 4096 * 3 + 5]


def _copy_few():
    out = [[Op(d, s, n)] for n in COPY_LENGTHS for d, s in COPY_PHASES]
    # a short range beside the one that sizes the grid, in every slot
    multi = [[524293, 1], [17, 262161, 4097], [4096, 0, 524293, 15], [1, 262144], [15, 16, 17, 4095]]
    for r, lens in enumerate(multi):
        for rot in range(3):
            ph = [COPY_PHASES[(i + rot + r) % len(COPY_PHASES)] for i in range(len(lens))]
            out.append([Op(d, s, n) for (d, s), n in zip(ph, lens)])
    return out


COPY_FEW = _copy_few()
COPY_MANY = [Op(0, s, n) for n in COPY_LENGTHS for s in COPY_SRC_PHASES]
COPY_TO_HOST = [Op(0, s, n) for n in HOST_LENGTHS for s in COPY_SRC_PHASES]


def copy_class(op, form, longest=None):
    """form "few" | "many" | "bg" | "host"; longest: the launch's longest range (it sizes the grid of "few" and
    "many").  The head (copy_few alone), how the 16-byte pieces are loaded, the grid's workgroups, the 16-byte pieces
    of the longest walk a thread makes (1: no stride) and the bytes of the last, partial piece."""
    longest = op.length if longest is None else longest
    head = head_of(op.dphase, op.length) if form == "few" else 0
    n = op.length - head
    cls = "x4" if form == "few" and (op.sphase + head) % 16 == 0 else "piece"
    wgs = {"few": min(-(-longest // COPY_WG_BYTES), COPY_MAX_WGS), "many": min(-(-longest // COPY_WG_BYTES), COPY_MAX_WGS),
           "bg": 1, "host": -(-op.length // COPY_WG_BYTES)}[form]
    pieces = -(-n // 16)
    return dict(head=head, cls=cls, wgs=wgs, strides=-(-pieces // (wgs * COPY_THREADS)) if wgs else 0, last=n % 16)


# ---- packing a table into buffers ----

Packed = namedtuple("Packed", "ops src_off dst_off src dst_size image edge_src edge_ops")


def pack(ops, key, edge=()):
    """Lays the ranges out: sources one after another at their phases in one buffer (`src`, distinct splitmix streams,
    SLACK bytes after the last), destinations at their phases in a buffer of dst_size bytes with at least GUARD
    bytes of FILL between two of them and at both ends.  image: the destination buffer after a correct launch.
    edge: indices of ranges whose sources go into a second buffer, edge_src, the last of them ending at its last
    byte.  src_off[i] is then an offset into edge_src (edge_ops says which)."""
    edge = list(edge)
    so, do, cur_s, cur_d, cur_e = [], [], 16, GUARD, 0
    for i, op in enumerate(ops):
        if i in edge:
            so.append(None)
        else:
            so.append(cur_s + op.sphase)
            cur_s = (cur_s + op.sphase + op.length + 15) & ~15
        do.append(cur_d + op.dphase)
        cur_d = (cur_d + op.dphase + op.length + GUARD + 15) & ~15
    src = np.full(cur_s + SLACK, 0x5A, np.uint8)
    image = np.full(cur_d + GUARD, FILL, np.uint8)
    for i in edge:  # packed so that the last one's last byte is the buffer's last
        so[i] = cur_e + ops[i].sphase
        cur_e = so[i] + ops[i].length
        if i != edge[-1]:
            cur_e = (cur_e + 15) & ~15
    edge_src = np.full(cur_e, 0x5A, np.uint8)
    for i, op in enumerate(ops):
        if op.length == 0:
            continue
        data = O.splitmix(op.length, key + 16 * i)
        (edge_src if i in edge else src)[so[i]:so[i] + op.length] = data
        image[do[i]:do[i] + op.length] = data
    return Packed(list(ops), so, do, src, image.size, image, edge_src, set(edge))


def shuffled(n, key):
    order = list(range(n))
    random.Random(key).shuffle(order)
    return order


def describe(op, T=None, D=None, form=None, longest=None):
    """A range with its class, for a failure's message."""
    if form is not None:
        return f"dst%16={op.dphase} src%16={op.sphase} len={op.length} {form} {copy_class(op, form, longest)}"
    return f"dst%16={op.dphase} src%16={op.sphase} len={op.length} <{T},{D}> {gather_class(op.sphase, op.dphase, op.length, T, D)}"


def mismatches(packed, got, limit=8):
    """Where a downloaded destination buffer differs from the image: the indices of the ranges that hold a wrong byte
    or whose following guard does (at most `limit`), and whether the leading guard is intact."""
    bad = np.flatnonzero(got != packed.image)
    if bad.size == 0:
        return [], True
    starts = np.array(packed.dst_off)
    return sorted({int(i) for i in np.searchsorted(starts, bad, side="right") - 1 if i >= 0})[:limit], bool(bad[0] >= starts[0])


# ---- the windows ----

WINDOW_R = [0, 16, 48, 64, 16384, 16432, 16448, 16464, 32768, 49216, 49232]
WINDOW_HEADS = [0, 1, 15]
WINDOW_BASES = [0, 1, 8]  # the file's first byte, from a 256-byte boundary
PATTERNS = ["splitmix", "hi", "x80", "x7f"]
SHORT_B = 700
SHORT_W = [1, 15, 16, 17, SHORT_B - 1]
BLOCK_BS = [512, 563, 20480]

# a window of the file (n bytes, block length B) at position p: w = min(B, n - p)
Window = namedtuple("Window", "B p n base pattern")


def pattern(name, n, key):
    if name == "x80":
        return np.full(n, 0x80, np.uint8)
    if name == "x7f":
        return np.full(n, 0x7F, np.uint8)
    out = O.splitmix(n, key)
    if name == "hi":  # every byte negative as a signed byte
        out |= 0x80
    else:
        assert name == "splitmix"
    return out


def _position(head):
    return 32 - head  # p % 16 = (16 - head) % 16, with bytes before it


def window_shapes():
    """(B, p, n) of the table.  Full windows: every B = head + R + tail, each at the three positions (a position's own
    head gives the window (head, R, tail); the other two give its neighbours), in a file of FILE_BYTES bytes.  Short
    windows: the file ends w bytes after p."""
    out = []
    for B in sorted({head + R + tail for R in WINDOW_R for head in WINDOW_HEADS for tail in TAILS} - {0}):
        for head in WINDOW_HEADS:
            out.append((B, _position(head), FILE_BYTES))
    for w in SHORT_W:
        for head in WINDOW_HEADS:
            out.append((SHORT_B, _position(head), _position(head) + w))
    return out


FILE_BYTES = 32 + max(WINDOW_R) + 30 + 5  # one file per (pattern, base) holds every window, 5 bytes after the longest
WINDOWS = [Window(B, p, n, base, pat) for pat in PATTERNS for base in WINDOW_BASES for B, p, n in window_shapes()]


def window_launches():
    """[(pattern, base, B, n, [windows])]: the table's windows by launch -- one file and one block length each."""
    out = {}
    for c in WINDOWS:
        out.setdefault((c.pattern, c.base, c.B, c.n), []).append(c)
    return [k + (v,) for k, v in out.items()]


BlockFile = namedtuple("BlockFile", "B n base pattern")
BLOCK_FILES = [BlockFile(B, 5 * B + r, WINDOW_BASES[i % 3], PATTERNS[i % 4])
               for i, (B, r) in enumerate((B, r) for B in BLOCK_BS for r in (0, 1, B - 1))]


def window_class(p, w, T=WINDOW_THREADS):
    """range_sums over [p, p + w) at T threads: head bytes, the 16-byte region R, tail bytes, thread 0's iterations of
    the eight-load loop, how many threads take one, the bytes of the piece loop's last piece (0: none is short)."""
    head = min(w, (16 - p % 16) % 16)
    R = (w - head) & ~15
    first = 64 * T + 64  # thread t enters when 64 t + first <= R
    it0 = 0 if R < first else (R - first) // (128 * T) + 1
    threads = 0 if R < first else min(T, (R - first) // 64 + 1)
    return dict(head=head, R=R, tail=w - head - R, unrolled0=it0, unrolled_threads=threads, last_piece=R % 64)


def window_id(c):
    w = min(c.B, c.n - c.p)
    return f"B{c.B}-p{c.p}-w{w}-base{c.base}-{c.pattern} {window_class(c.p, w)}"


def weak_sum(x):
    """The weak sum of the window x (uint8 array) in closed form: S1 = sum sbyte(x_j), S2 = sum (w - j) sbyte(x_j),
    T = (S1 & 0xFFFF) | (S2 & 0xFFFF) << 16 as int32.  Exact: the sums stay far below 2^63."""
    v = x.view(np.int8).astype(np.int64)
    w = v.size
    s1 = int(v.sum())
    s2 = int((v * np.arange(w, 0, -1, dtype=np.int64)).sum())
    t = (s1 & 0xFFFF) | ((s2 & 0xFFFF) << 16)
    return t - (1 << 32) if t >= 1 << 31 else t


_FILES = {}


def window_file(name):
    """The FILE_BYTES bytes that every window of a pattern is cut from (read-only, computed once)."""
    if name not in _FILES:
        a = pattern(name, FILE_BYTES, 0x5EED5EED10C40000 + PATTERNS.index(name))
        a.setflags(write=False)
        _FILES[name] = a
    return _FILES[name]


_WANT = {}


def window_want(c):
    """The closed form of a table window (the base does not enter), computed once."""
    k = (c.B, c.p, c.n, c.pattern)
    if k not in _WANT:
        _WANT[k] = weak_sum(window_file(c.pattern)[c.p:c.p + min(c.B, c.n - c.p)])
    return _WANT[k]


def block_file(f):
    return pattern(f.pattern, f.n, 0x5EED5EED10C4B000 + f.B + f.n)


# ---- the constants, read back from the kernels' source ----

def source_constants(text):
    """What device_io.hip's launchers say where this module has constants: the two gather instantiations and their
    switch, the copies' bytes per workgroup and workgroup limit, window_weak_kernel's threads."""
    forms = [(int(t), int(d)) for t, d in re.findall(r"gather_ops_kernel_t<(\d+), (\d+), true, true>\), dim3\(n\), dim3\(\1\)",
                                                     text.split("#ifdef RSH_KBENCH")[0])]
    switch = re.search(r"if \(avg_len < \((\d+) << (\d+)\)\)", text)
    few = re.search(r"hipError_t launch_copy_few\(.*?std::min<int64_t>\(\(mx \+ (\d+) \* (\d+) - 1\) / \(\1 \* \2\), (\d+)\);.*?"
                    r"dim3\(\(uint32_t\)blocks, f\.n\), dim3\((\d+)\)", text, re.S)
    many = re.search(r"hipError_t launch_copy_many\(.*?bg \? 1 : std::min<int64_t>\(\(max_len \+ (\d+) \* (\d+) - 1\) / "
                     r"\(\1 \* \2\), (\d+)\);.*?dim3\(\(uint32_t\)blocks, n\), dim3\((\d+)\)", text, re.S)
    win = re.search(r"hipLaunchKernelGGL\(window_weak_kernel, dim3\(n\), dim3\((\d+)\)", text)
    return dict(forms=forms, switch=int(switch.group(1)) << int(switch.group(2)),
                few=(int(few.group(1)) * int(few.group(2)), int(few.group(3)), int(few.group(4))),
                many=(int(many.group(1)) * int(many.group(2)), int(many.group(3)), int(many.group(4))),
                window_threads=int(win.group(1)))
