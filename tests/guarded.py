"""Guarded arrays for the memory contract of the C-ABI operators: every array an operator sees sits inside a larger allocation
of its own whose bytes in front of and behind the payload hold a known pattern, so that a store outside an output, a use of
workspace beyond the advertised bytes or a modified input is REPORTED by ``Arena.verify()`` instead of landing in the
allocator's slack or in an unrelated tensor.  A plain helper module (not a conftest): tests/test_guarded_host.py shows on host
tensors that the checker can fail, tests/test_gpu_memory_contract.py runs every entry point through it on the device.

Guard size -- a SAFETY condition, not a tuning knob.  The front guard is 4 KiB (plus the element offset); the rear guard is
max(1 MiB, payload bytes), capped at 64 MiB.  A kernel that overruns an array by up to that array's own size therefore still
writes inside memory this module owns: the test detects the overrun and fails, it does not fault the card.  Do not shrink it.

Patterns.  Outputs, workspaces and the guards of floating-point inputs are 0xFF bytes: a NaN as float16 / float32 / float64, so
a read past the end that enters the arithmetic poisons the result even when it is multiplied by zero, and a workspace whose
contents are consumed before they are written shows in the output.  Integer inputs (indices, lengths, tokens, maps) and int8
Rademacher arrays get guards of 0: a valid index -- an out-of-range read of one must never turn into a wild address -- and a
sign that is neither +1 nor -1, which zeroes a term.

``Plain`` offers the same three methods over separately allocated tensors, the way the value tests allocate them, so that one
piece of code runs an operator both ways."""
import ctypes

import torch

FRONT_GUARD = 4096
REAR_GUARD_MIN = 1 << 20
REAR_GUARD_MAX = 64 << 20
ALIGN = 256
POISON = 0xFF
STUB = 16               # bytes behind a zero-byte workspace: non-null, 16-byte aligned, all of it guard


def rear_guard_bytes(payload_bytes):
    return min(max(REAR_GUARD_MIN, int(payload_bytes)), REAR_GUARD_MAX)


def _nelem(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def bits(t):
    """The bytes of a tensor as a flat uint8 view (contiguous tensors only)."""
    return t.contiguous().reshape(-1).view(torch.uint8)


def same_bits(a, b):
    """Bit-for-bit equality: -0 and NaN payloads count."""
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


class _Record:
    __slots__ = ("name", "kind", "buf", "start", "end", "guard", "copy")

    def __init__(self, name, kind, buf, start, end, guard, copy=None):
        self.name, self.kind, self.buf, self.start, self.end, self.guard, self.copy = name, kind, buf, start, end, guard, copy


class Plain:
    """The allocator of the plain run: separate tensors of exactly their size, as the value tests allocate them."""

    def __init__(self, device):
        self.device = torch.device(device)

    def out(self, shape, dtype, fill=None, offset_elems=0, init=None, name=None):
        if init is not None:
            return init.detach().clone().to(self.device).reshape(shape).contiguous()
        if fill is None:
            t = torch.empty(shape, dtype=dtype, device=self.device)
            bits(t).fill_(POISON) if t.numel() else None
            return t
        return torch.full(shape, fill, dtype=dtype, device=self.device)

    def inp(self, tensor, offset_elems=0, guard="nan", name=None):
        return tensor.detach().clone().to(self.device).contiguous()

    def workspace(self, nbytes, name=None):
        return torch.empty(int(nbytes) if int(nbytes) > 0 else STUB, dtype=torch.uint8, device=self.device)

    def verify(self):
        pass


class Arena:
    """Guarded arrays on ``device`` ("cuda" or "cpu").  Every ``out`` / ``inp`` / ``workspace`` is a view into an allocation of
    its own; ``verify()`` checks all of them at once."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.records = []

    # ------------------------------------------------------------------------------------------------ allocation
    def _carve(self, nbytes, offset_bytes, guard_byte, rear_payload=None):
        """-> (buf, start): a uint8 buffer filled with guard_byte and the payload's first byte, 256-byte aligned + offset."""
        rear = rear_guard_bytes(nbytes if rear_payload is None else rear_payload)
        total = ALIGN + FRONT_GUARD + offset_bytes + nbytes + rear
        buf = torch.empty(total, dtype=torch.uint8, device=self.device)
        buf.fill_(guard_byte)
        start = (-buf.data_ptr()) % ALIGN + FRONT_GUARD + offset_bytes
        assert FRONT_GUARD % ALIGN == 0 and start + nbytes + rear <= total
        return buf, start

    def _view(self, buf, start, shape, dtype):
        nbytes = _nelem(shape) * torch.empty((), dtype=dtype).element_size()
        return buf[start:start + nbytes].view(dtype).reshape(tuple(int(s) for s in shape))

    def _name(self, name, kind):
        return name if name is not None else f"{kind}#{len(self.records)}"

    def out(self, shape, dtype, fill=None, offset_elems=0, init=None, name=None):
        """A contiguous view of ``shape`` with 0xFF guards; payload = ``fill``, or 0xFF bytes, or -- for an in-place operand --
        the bits of ``init``.  Only the guards are checked."""
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        item = torch.empty((), dtype=dtype).element_size()
        nbytes = _nelem(shape) * item
        buf, start = self._carve(nbytes, int(offset_elems) * item, POISON)
        view = self._view(buf, start, shape, dtype)
        if init is not None:
            assert init.dtype == dtype and init.numel() == view.numel()
            view.copy_(init.detach().to(self.device).reshape(shape))
        elif fill is not None:
            view.fill_(fill)
        self.records.append(_Record(self._name(name, "out"), "out", buf, start, start + nbytes, POISON))
        return view

    def inp(self, tensor, offset_elems=0, guard="nan", name=None):
        """A guarded copy of an input; the arena keeps a private bit copy.  guard "nan": 0xFF bytes for floating-point data;
        integer data (indices, lengths, tokens, signs) always gets guards of 0, as does guard "zero"."""
        assert guard in ("nan", "zero")
        src = tensor.detach().contiguous()
        guard_byte = POISON if (guard == "nan" and src.dtype.is_floating_point) else 0
        nbytes = src.numel() * src.element_size()
        buf, start = self._carve(nbytes, int(offset_elems) * src.element_size(), guard_byte)
        view = self._view(buf, start, tuple(src.shape), src.dtype)
        view.copy_(src.to(self.device))
        copy = buf[start:start + nbytes].clone()
        self.records.append(_Record(self._name(name, "inp"), "inp", buf, start, start + nbytes, guard_byte, copy))
        return view

    def workspace(self, nbytes, name=None, _registered=None):
        """A uint8 view of exactly ``nbytes`` bytes, 256-byte aligned, 0xFF-filled, guarded on both sides; for 0 bytes a 16-byte
        stub all of which is guard.  (``_registered``: the bytes the arena treats as payload -- the negative control's lie.)"""
        nbytes = int(nbytes)
        span = nbytes if nbytes > 0 else STUB
        buf, start = self._carve(span, 0, POISON)
        owned = nbytes if _registered is None else int(_registered)
        self.records.append(_Record(self._name(name, "workspace"), "workspace", buf, start, start + owned, POISON))
        return buf[start:start + span]

    # ------------------------------------------------------------------------------------------------ the check
    @staticmethod
    def _changed(region, value):
        bad = torch.nonzero(region != value).reshape(-1)
        return (int(bad[0]), int(bad[-1])) if bad.numel() else None

    def violations(self):
        """-> list of messages, one per damaged guard / modified input (empty: the contract held)."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        flags = []
        for r in self.records:
            flags.append((r.buf[:r.start] != r.guard).any())
            flags.append((r.buf[r.end:] != r.guard).any())
            flags.append((r.buf[r.start:r.end] != r.copy).any() if r.copy is not None else torch.zeros((), dtype=torch.bool,
                                                                                                        device=self.device))
        if not flags or not bool(torch.stack(flags).any()):
            return []
        flags = torch.stack(flags).cpu().tolist()
        msgs = []
        for i, r in enumerate(self.records):
            size = r.end - r.start
            if flags[3 * i]:
                lo, hi = self._changed(r.buf[:r.start], r.guard)
                msgs.append(f"{r.name} ({r.kind}, {size} bytes): front guard changed, bytes {lo - r.end} .. {hi - r.end} "
                            f"relative to the payload's end")
            if flags[3 * i + 1]:
                lo, hi = self._changed(r.buf[r.end:], r.guard)
                msgs.append(f"{r.name} ({r.kind}, {size} bytes): rear guard changed, bytes +{lo} .. +{hi} "
                            f"relative to the payload's end")
            if flags[3 * i + 2]:
                bad = torch.nonzero(r.buf[r.start:r.end] != r.copy).reshape(-1)
                msgs.append(f"{r.name} (inp, {size} bytes): input modified, bytes {int(bad[0]) - size} .. {int(bad[-1]) - size} "
                            f"relative to the payload's end")
        return msgs

    def verify(self):
        msgs = self.violations()
        assert not msgs, "memory contract violated:\n  " + "\n  ".join(msgs)


def patched_workspaces(monkeypatch, ext, arena):
    """Replaces ``ext._workspace`` -- the one seam through which the wrappers allocate their internal workspaces, which rounds
    up to 256 bytes -- by one that hands out exactly the bytes the library's *_workspace_bytes function asked for, from the
    arena.  (Wrappers that take ``workspace=None`` allocate on their own: give those an explicit ``arena.workspace(need)``.)
    The device copy of the host sequence lengths, which the sequence wrappers make through ``ext._seqlens``, becomes a guarded
    input as well (guards of 0: a length that is read past the end starts no k-mer loop)."""
    def exact(nbytes, device):
        nbytes = int(nbytes)
        ws = arena.workspace(nbytes, name=f"internal workspace#{len(arena.records)}")
        return ws, ctypes.c_void_p(ws.data_ptr()), ctypes.c_size_t(nbytes)
    monkeypatch.setattr(ext, "_workspace", exact)
    seqlens = getattr(ext, "_seqlens", None)
    if seqlens is not None:
        def guarded_seqlens(seqlengths, device):
            host, dev = seqlens(seqlengths, device)
            return host, arena.inp(dev, name=f"device sequence lengths#{len(arena.records)}")
        monkeypatch.setattr(ext, "_seqlens", guarded_seqlens)
