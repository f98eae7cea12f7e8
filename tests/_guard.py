"""Guard-banded buffers for the kernel tests (test infrastructure, not a conftest).

`GuardedBackend` wraps a `conftest.Backend` and hands out every buffer (`t`, `empty`, `zeros`, `empty_int`) as a contiguous
view into a larger flat allocation: the view starts on a 256-byte boundary and sits between two guard bands of at least
max(64 KiB, size of the buffer) each.  Float guards hold a repeating tagged NaN, +3e38, -3e38 (NaN poisons a sum that reads it,
the huge values poison max / arg-max, which ignore NaN); integer guards hold 0xA5 bytes.  `call(name, ...)`:

* snapshots every registered buffer that a `const` pointer argument of `name` points into (const-ness is read from
  include/monkeynet_hip.h here: mnk/_lib.py drops it), unless a non-const argument of the same call points into it too;
* runs the entry point and synchronises;
* checks that those buffers are unchanged and that the guards of every buffer of the call are intact, byte for byte.

Every guard is checked again at teardown.  Nothing is checked while a stream is capturing.  A reported offset is counted from
the end of the view (a guard after it) or from its start (a guard in front: a negative offset).

`ws_shrink = 1` runs every entry point that takes `(ws, ws_floats)` on a workspace one float smaller than the caller's: the
kernel gets a fresh guarded buffer of ws_floats - 1 floats (guards >= the full size, so an unchecked overrun lands in owned
memory) and must either raise MnkError -- the call is then repeated with the caller's workspace -- or succeed; `ws_log`
records (name, ws_floats, "exact" | "raised" | "ran") of every call with a non-empty workspace.

The pytest fixture `be` below overrides the conftest fixture of the same name in every module that imports it, and keeps its
emu / hip parameters and gpu marks."""
import os
import re

import numpy as np
import pytest
import torch

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "monkeynet_hip.h")
ALIGN = 256
MIN_GUARD = 64 * 1024
FLOAT_GUARD = np.array([0x7FC5A5A5, np.float32(3e38).view(np.uint32), np.float32(-3e38).view(np.uint32)], dtype=np.uint32)
INT_GUARD = 0xA5


def parse_pointer_args(path=HEADER):
    """{entry point: [(argument name, 'const' | 'mut' | None)]} for every function of the header; 'const' = pointer to const"""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"#.*", "", text)
    out = {}
    for m in re.finditer(r"(?:const\s+char\s*\*|int|size_t)\s+(mnk_\w+)\s*\(([^)]*)\)\s*;", text):
        args = m.group(2).strip()
        spec = []
        if args and args != "void":
            for a in args.split(","):
                a = " ".join(a.split())
                name = re.search(r"(\w+)$", a).group(1)
                ty = a[: a.rfind(name)].strip()
                spec.append((name, ("const" if ty.startswith("const") else "mut") if "*" in ty else None))
        out[m.group(1)] = spec
    return out


_SPECS = {}


def _spec(name):
    if not _SPECS:
        _SPECS.update(parse_pointer_args())
    return _SPECS[name]


def _round_up(v, a):
    return (v + a - 1) // a * a


_PATTERNS = {}


def _pattern(device, is_float, nbytes):
    """a cached flat byte pattern of at least nbytes on `device` (guards are compared against the same bytes)"""
    key = (str(device), is_float)
    p = _PATTERNS.get(key)
    if p is None or p.numel() < nbytes:
        n = _round_up(max(nbytes, 1 << 20) * 2, 12)
        if is_float:
            host = torch.from_numpy(np.tile(FLOAT_GUARD, n // 12).view(np.uint8))
        else:
            host = torch.full((n,), INT_GUARD, dtype=torch.uint8)
        p = _PATTERNS[key] = host.to(device)
    return p


class _Buf:
    __slots__ = ("flat", "off", "nbytes", "is_float", "start", "end")

    def __init__(self, flat, off, nbytes, is_float):
        self.flat, self.off, self.nbytes, self.is_float = flat, off, nbytes, is_float
        self.start = flat.data_ptr() + off
        self.end = self.start + nbytes

    def view_bytes(self):
        return self.flat[self.off:self.off + self.nbytes]

    def first_bad_guard(self):
        """None, or the corrupted byte nearest to the view: (offset from the end of the view (>= 0) or from its start (< 0), value)"""
        pat = _pattern(self.flat.device, self.is_float, self.flat.numel())
        hi = self.off + self.nbytes
        after, before = self.flat[hi:], self.flat[:self.off]
        if not torch.equal(after, pat[hi:self.flat.numel()]):
            k = int((after != pat[hi:self.flat.numel()]).nonzero()[0, 0])
            return k, self._word(hi + k)
        if not torch.equal(before, pat[:self.off]):
            k = int((before != pat[:self.off]).nonzero()[-1, 0])
            return k - self.off, self._word(k)
        return None

    def _word(self, byte):
        w = byte // 4 * 4
        v = self.flat[w:w + 4].cpu()
        return "bytes %s = %r as float" % (v.tolist(), float(v.view(torch.float32)[0])) if v.numel() == 4 else str(v.tolist())


class GuardedBackend:
    """A conftest.Backend whose buffers carry guard bands and whose calls are checked (module docstring)."""

    def __init__(self, inner):
        self._be = inner
        self._bufs = []
        self.ws_shrink = 0
        self.ws_log = []

    def __getattr__(self, name):            # kind, lib, device, stream, query, sync, ...
        return getattr(self._be, name)

    # ---- allocation ---------------------------------------------------------------------------------------------------------
    def _alloc(self, shape, dtype):
        shape = tuple(int(s) for s in (shape[0] if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size))
                                       else shape))
        n = 1
        for s in shape:
            n *= s
        esize = torch.empty((), dtype=dtype).element_size()
        nbytes = n * esize
        is_float = dtype == torch.float32
        guard = _round_up(max(MIN_GUARD, nbytes), ALIGN)
        total = guard + ALIGN + _round_up(nbytes, ALIGN) + guard
        flat = _pattern(self.device, is_float, total)[:total].clone()
        off = _round_up(flat.data_ptr() + guard, ALIGN) - flat.data_ptr()
        buf = _Buf(flat, off, nbytes, is_float)
        self._bufs.append(buf)
        return flat[off:off + nbytes].view(dtype).view(shape)

    def t(self, x):
        x = x.contiguous()
        out = self._alloc(x.shape, x.dtype)
        out.copy_(x)
        return out

    def empty(self, *shape):
        return self._alloc(shape, torch.float32).fill_(float("nan"))

    def zeros(self, *shape):
        return self._alloc(shape, torch.float32).zero_()

    def empty_int(self, *shape, dtype=torch.int32):
        """an integer / byte buffer whose contents are 0x5A bytes (a missing write shows), guards 0xA5"""
        out = self._alloc(shape, dtype)
        out.view(torch.uint8).fill_(0x5A)
        return out

    # ---- checked calls ------------------------------------------------------------------------------------------------------
    def _find(self, ptr):
        for b in self._bufs:
            if b.start <= ptr < b.end or (ptr == b.start and b.nbytes == 0):
                return b
        return None

    def _capturing(self):
        return self.kind == "hip" and torch.cuda.is_current_stream_capturing()

    def call(self, name, *args):
        if self._capturing():
            return self._be.call(name, *args)
        spec = _spec(name)
        assert len(spec) == len(args) + 1 and spec[-1][0] == "stream", (name, len(args), spec)
        uses = {}                                            # id(buf) -> (buf, [(arg name, kind)])
        for (aname, kind), a in zip(spec, args):
            if kind is not None and torch.is_tensor(a):
                b = self._find(a.data_ptr())
                if b is not None:
                    uses.setdefault(id(b), (b, []))[1].append((aname, kind))
        snaps = [(b, [n for n, _ in u], b.view_bytes().clone()) for b, u in uses.values() if all(k == "const" for _, k in u)]
        shrink = self._shrunk_workspace(name, spec, args)
        err = None
        try:
            if shrink is None:
                self._be.call(name, *args)
            else:
                self._call_shrunk(name, spec, args, *shrink)
        except Exception as e:          # the guards are checked first: a corrupted neighbour is the finding, not the error
            err = e
        self._be.sync()
        for b, names, snap in snaps:
            if not torch.equal(b.view_bytes(), snap):
                k = int((b.view_bytes() != snap).nonzero()[0, 0])
                raise AssertionError("%s wrote through const argument %s: byte %d of the view changed" % (name, "/".join(names), k))
        for b, u in uses.values():
            bad = b.first_bad_guard()
            if bad is not None:
                raise AssertionError("%s corrupted the guard of argument %s at byte offset %+d %s the view (%s)" % (
                    name, "/".join(n for n, _ in u), bad[0], "past the end of" if bad[0] >= 0 else "before the start of", bad[1]))
        if err is not None:
            raise err

    def _shrunk_workspace(self, name, spec, args):
        names = [n for n, _ in spec]
        if "ws" not in names or "ws_floats" not in names:
            return None
        i, j = names.index("ws"), names.index("ws_floats")
        if not torch.is_tensor(args[i]) or int(args[j]) <= self.ws_shrink:
            return None
        if not self.ws_shrink:
            self.ws_log.append((name, int(args[j]), "exact"))
            return None
        return i, j

    def _call_shrunk(self, name, spec, args, i, j):
        from mnk._lib import MnkError
        full = int(args[j])
        n = full - self.ws_shrink
        ws = args[i]
        small = self._alloc((n,), torch.float32)
        small.copy_(ws.reshape(-1)[:n])
        a = list(args)
        a[i], a[j] = small, n
        try:
            self._be.call(name, *a)
        except MnkError:
            self.ws_log.append((name, full, "raised"))
            self._be.call(name, *args)
            return
        self._be.sync()
        bad = self._find(small.data_ptr()).first_bad_guard()
        if bad is not None:
            raise AssertionError("%s wrote past a workspace of %d floats (queried %d): guard byte offset %+d (%s)" % (
                name, n, full, bad[0], bad[1]))
        ws.reshape(-1)[:n].copy_(small)
        self.ws_log.append((name, full, "ran"))

    def check_all(self, where="teardown"):
        self._be.sync()
        for b in self._bufs:
            bad = b.first_bad_guard()
            if bad is not None:
                raise AssertionError("%s: a guard of a %d-byte buffer is corrupted at byte offset %+d %s the view (%s)" % (
                    where, b.nbytes, bad[0], "past the end of" if bad[0] >= 0 else "before the start of", bad[1]))


def guarded(inner):
    return GuardedBackend(inner)


@pytest.fixture
def be(be):
    """the conftest backend (emu / hip) with guard-banded buffers and checked calls"""
    g = GuardedBackend(be)
    yield g
    if not g._capturing():
        g.check_all()
