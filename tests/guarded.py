"""Guard bands and poison for the buffers a caller hands to the C interface (include/ucdir_hip.h).

``Arena`` is one buffer between two guard bands, at exactly the alignment the header promises and filled with a poison byte;
``run_contract`` calls an entry point on such buffers once per poison byte and asserts, in this order, that no guard changed, that
no input changed, that the defined output bytes do not depend on the poison, and that they equal what the project's Python wrapper
returns.  Every assertion is an equality of bytes.  Works on CPU tensors too (tests/test_memory_contract_cpu.py models the faults
it has to report there); a plain module like hip_checks.py, no pytest setting."""
import ctypes

import numpy as np
import torch

GUARD_MIN = 4096
FILLS = (0xFF, 0xA5)      # 0xFF: NaN as fp32 / fp64, -1 as integers; 0xA5: finite garbage.  Neither is zero.


class ContractError(AssertionError):
    """A broken buffer contract.  ``kind``: "guard", "input", "fill" (a defined output byte depends on the poison: unwritten, or
    computed from unwritten memory) or "wrapper" (the output is not the Python wrapper's)."""

    def __init__(self, kind, message):
        super().__init__(f"[{kind}] {message}")
        self.kind = kind


class Arena:
    """[front guard | payload of ``nbytes`` | back guard] in ONE uint8 tensor on ``device``, every byte ``fill``.  Each guard has
    at least max(4096, nbytes) bytes: an overrun of a whole payload still lands in memory the test owns.  The payload starts at an
    address a with a % align == 0 and a % (2 align) == align: what the header promises and no more."""

    def __init__(self, nbytes, align, fill, device="cpu"):
        nbytes, align = int(nbytes), int(align)
        assert nbytes >= 0 and align >= 1 and align & (align - 1) == 0 and 0 <= fill <= 255
        self.nbytes, self.align, self.fill = nbytes, align, fill
        guard = max(GUARD_MIN, nbytes)
        self.buf = torch.full((2 * guard + nbytes + 2 * align,), fill, dtype=torch.uint8, device=device)
        base = self.buf.data_ptr()
        self.start = guard + (align - (base + guard)) % (2 * align)
        self.ptr = base + self.start
        assert self.ptr % align == 0 and self.ptr % (2 * align) == align
        assert self.start >= guard and self.buf.numel() - self.start - nbytes >= guard

    @property
    def payload(self):
        return self.buf[self.start:self.start + self.nbytes]

    def view(self, dtype, shape):
        """The payload as a tensor of ``dtype`` and ``shape`` (which must fill it)."""
        return self.payload.view(dtype).view(shape)

    def upload(self, t):
        """Copy the bytes of tensor ``t`` (any dtype and stride) into the payload."""
        src = as_bytes(t)
        assert src.numel() == self.nbytes, (src.numel(), self.nbytes)
        self.payload.copy_(src.to(self.buf.device))

    def bytes(self):
        """The payload on the host, a numpy uint8 array (a copy)."""
        return self.payload.cpu().numpy().copy()

    def check_guards(self, name="buffer"):
        """Both guards against ``fill``, byte for byte; call it after torch.cuda.synchronize().  Names the first changed offset
        relative to the payload (negative: in front of it)."""
        end = self.start + self.nbytes
        for lo, hi, what in ((0, self.start, "front"), (end, self.buf.numel(), "back")):
            bad = (self.buf[lo:hi] != self.fill).nonzero()
            if bad.numel():
                at = lo + int(bad[0]) - self.start
                where = f"{-at} bytes in front of the payload" if at < 0 else f"{at - self.nbytes} bytes behind the payload's end"
                raise ContractError("guard", f"{name}: the {what} guard of the {self.nbytes}-byte payload (alignment {self.align}, "
                                             f"fill {self.fill:#04x}) changed at payload offset {at} ({where}); "
                                             f"{int(bad.numel())} guard bytes changed")


def as_bytes(t):
    """The bytes of a tensor in memory order of its contiguous form, as a flat uint8 tensor."""
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t))
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


class In:
    """An input: the tensor whose bytes are uploaded, and the alignment the header promises for it."""

    def __init__(self, tensor, align):
        self.tensor, self.align = tensor, align


class Out:
    """An output of ``dtype`` and ``shape`` at ``align``.  ``init``: a tensor of that many bytes for an in-place argument (its
    bytes stand in the payload before the call; the guards keep the poison)."""

    def __init__(self, dtype, shape, align, init=None):
        self.dtype, self.shape, self.align, self.init = dtype, tuple(shape), align, init
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()


class Ws:
    """A workspace of ``nbytes`` at ``align``."""

    def __init__(self, nbytes, align):
        self.nbytes, self.align = int(nbytes), align


def _first_diff(a, b, mask=None):
    d = a != b
    if mask is not None:
        d &= mask
    idx = np.flatnonzero(d)
    return (int(idx[0]), int(idx.size)) if idx.size else None


def run_contract(call, inputs, outputs, workspaces=None, fills=FILLS, expect=None, mask=None, device="cuda"):
    """Run ``call`` once per poison byte of ``fills`` on guarded buffers and assert the buffer contract.

    ``inputs``: name -> In; ``outputs``: name -> Out; ``workspaces``: name -> Ws.  ``call(bufs)`` gets name -> Arena of all of
    them and calls the C function with ``ptr(bufs[name])`` (through lib.load(), as the tests' raw() helpers do); a non-zero return
    value raises the library's error.  ``expect``: name -> tensor, what the Python wrapper returns for the same inputs (or a
    callable that returns that dict); ``mask(outs)``: name -> boolean numpy array over an output's bytes, True where the header
    defines them, computed from the outputs' bytes ``outs`` (name -> numpy uint8) of one run.

    In order: every guard is intact; every input payload is what was uploaded; the defined output bytes are the same for every
    fill; they equal ``expect``.  Returns name -> tensor, the outputs of the last run."""
    workspaces = workspaces or {}
    assert len(fills) >= 2 and not (set(inputs) & set(outputs)) and not (set(workspaces) & (set(inputs) | set(outputs)))
    runs = []
    for fill in fills:
        bufs = {}
        for name, spec in inputs.items():
            src = as_bytes(spec.tensor)
            bufs[name] = Arena(src.numel(), spec.align, fill, device)
            bufs[name].upload(spec.tensor)
        for name, spec in outputs.items():
            bufs[name] = Arena(spec.nbytes, spec.align, fill, device)
            if spec.init is not None:
                bufs[name].upload(spec.init)
        for name, spec in workspaces.items():
            bufs[name] = Arena(spec.nbytes, spec.align, fill, device)
        rc = call(bufs)
        if torch.device(device).type == "cuda":
            torch.cuda.synchronize()
        if rc:
            from ucdir_amd import lib
            lib.check(rc)
        for name, a in bufs.items():
            a.check_guards(f"{name} (fill {fill:#04x})")
        for name, spec in inputs.items():
            hit = _first_diff(bufs[name].bytes(), as_bytes(spec.tensor).cpu().numpy())
            if hit:
                raise ContractError("input", f"input {name} (fill {fill:#04x}) changed: first at byte {hit[0]}, {hit[1]} bytes in all")
        outs = {name: bufs[name].bytes() for name in outputs}
        m = mask(outs) if mask is not None else {}
        runs.append((fill, outs, {k: np.asarray(v, bool).reshape(-1) for k, v in m.items()}, bufs))
    fill0, outs0, mask0, _ = runs[0]
    for fill, outs, m, _ in runs[1:]:
        for name in outputs:
            if (name in mask0) != (name in m) or (name in m and not np.array_equal(mask0[name], m[name])):
                raise ContractError("fill", f"output {name}: the defined bytes differ between fill {fill0:#04x} and {fill:#04x}")
            hit = _first_diff(outs0[name], outs[name], mask0.get(name))
            if hit:
                raise ContractError("fill", f"output {name}: fill {fill0:#04x} and fill {fill:#04x} give different bytes, first at byte "
                                            f"{hit[0]} ({outs0[name][hit[0]]:#04x} against {outs[name][hit[0]]:#04x}), {hit[1]} in all: "
                                            "unwritten, or computed from memory the call never wrote")
    if expect is not None:
        want = expect() if callable(expect) else expect
        assert set(want) <= set(outputs), (set(want), set(outputs))
        for name, t in want.items():
            w = as_bytes(t).cpu().numpy()
            if w.size != outs0[name].size:
                raise ContractError("wrapper", f"output {name}: {outs0[name].size} bytes, the wrapper returns {w.size}")
            hit = _first_diff(outs0[name], w, mask0.get(name))
            if hit:
                raise ContractError("wrapper", f"output {name} is not the wrapper's: first at byte {hit[0]} ({outs0[name][hit[0]]:#04x} "
                                               f"against {w[hit[0]]:#04x}), {hit[1]} bytes in all")
    last = runs[-1][3]
    return {name: last[name].view(spec.dtype, spec.shape).clone() for name, spec in outputs.items()}


def ptr(a, offset=0):
    """An arena's payload address (plus ``offset`` bytes) as ctypes hands it to the C interface; None is the null pointer."""
    return ctypes.c_void_p(0) if a is None else ctypes.c_void_p(a.ptr + int(offset))


class HostArena:
    """The same for the host-only functions: a numpy uint8 buffer [guard | payload | guard], every byte ``fill``."""

    def __init__(self, nbytes, fill=0xA5, align=8):
        self.nbytes, self.fill = int(nbytes), fill
        guard = max(GUARD_MIN, self.nbytes)
        self.buf = np.full(2 * guard + self.nbytes + 2 * align, fill, np.uint8)
        base = self.buf.ctypes.data
        self.start = guard + (align - (base + guard)) % (2 * align)
        self.ptr = base + self.start

    @property
    def payload(self):
        return self.buf[self.start:self.start + self.nbytes]

    def view(self, dtype):
        return self.payload.view(dtype)

    def written(self):
        """Offsets (relative to the payload) of every byte of the WHOLE buffer that is no longer ``fill``."""
        return np.flatnonzero(self.buf != self.fill) - self.start

    def guards_intact(self):
        w = self.written()
        return not ((w < 0) | (w >= self.nbytes)).any()
