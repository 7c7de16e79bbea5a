"""The guarded arena of tests/test_gpu_hotpath_overlap.py and tests/test_gpu_containment.py, and the three-run containment check built on it.

One uint8 allocation filled with a canary byte; every buffer a call sees is a view into it, with GUARD bytes of canary in front of the
first, between any two and behind the last.  A stray store lands in a guard band or in another operand and changes a byte the
snapshot holds; a stray load that reaches a result takes the canary with it, and two runs with different canaries then differ.
Plain torch: the class works on any device (tests/test_containment_host.py runs it on the CPU).

Roles of a buffer:
  "in"   must be byte-identical after the call;
  "out"  may be written; its bytes are compared between runs;
  "ws"   may be written; its bytes are never compared.
An "out" or "ws" buffer starts as the canary unless `like=` gives it contents (an accumulate-into-zeros output, a workspace the
contract wants zeroed, an output the contract writes only in part)."""
import numpy as np
import torch

CANARY = 0xA5          # as float32 about -2.9e-16, as int32 / int64 a large negative number
CANARY_B = 0xFF        # NaN as float32 / float64, -1 as any integer
PLAIN = 0x3C           # what an output without contents starts with in the unguarded run (ordinary allocations)
GUARD = 64 * 1024
ROLES = ("in", "out", "ws")


class Arena:
    """One uint8 allocation filled with `fill`; every buffer a kernel sees is a view into it, with GUARD bytes of it in front
    of the first, between any two and behind the last.  add() before build(); check() after the launches."""

    def __init__(self, fill=CANARY):
        assert 0 <= int(fill) <= 255
        self.fill = int(fill)
        self.specs, self.total, self.buf, self.snap = [], GUARD, None, None

    def add(self, name, like=None, shape=None, dtype=None, out=False, role=None):
        """like: a tensor whose contents the buffer starts with (an input, or an output the caller wants pre-filled);
        shape/dtype: a buffer left full of canary bytes.  out=True: the launches may write it (role "out"); role: "in", "out" or
        "ws" (overrides `out`)."""
        role = role or ("out" if out else "in")
        assert role in ROLES, role
        shape = tuple(like.shape) if like is not None else tuple(shape)
        dtype = like.dtype if like is not None else dtype
        nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
        spec = dict(name=name, off=self.total, nbytes=nbytes, shape=shape, dtype=dtype, like=like, role=role, out=role != "in")
        self.specs.append(spec)
        self.total += (nbytes + 255) // 256 * 256 + GUARD     # 256-byte aligned starts (the kernels want 16)
        return len(self.specs) - 1

    def build(self, dev):
        self.buf = torch.full((self.total,), self.fill, dtype=torch.uint8, device=dev)
        views = []
        for s in self.specs:
            v = self.buf[s["off"]:s["off"] + s["nbytes"]].view(s["dtype"]).view(s["shape"])
            if s["like"] is not None:
                v.copy_(s["like"])
            s["view"] = v
            views.append(v)
        self.snap = self.buf.clone()
        return views

    def reset_outputs(self):
        """refill every output with the bytes it had after build()"""
        for s in self.specs:
            if s["out"]:
                self.buf[s["off"]:s["off"] + s["nbytes"]].copy_(self.snap[s["off"]:s["off"] + s["nbytes"]])

    def check(self, what):
        """every byte that is not inside a declared output -- guard bands, inputs, weights -- is what it was after build()"""
        changed = self.buf != self.snap
        for s in self.specs:
            if s["out"]:
                changed[s["off"]:s["off"] + s["nbytes"]] = False
        n = int(changed.sum())
        if n == 0:
            return
        first = int(torch.nonzero(changed)[0])
        last = int(torch.nonzero(changed)[-1])
        where = "the leading guard band"
        for s in self.specs:
            if first >= s["off"]:
                where = (f"{s['name']} at byte {first - s['off']} of {s['nbytes']}" if first < s["off"] + s["nbytes"]
                         else f"the guard band {first - s['off'] - s['nbytes']} bytes behind {s['name']}")
        raise AssertionError(f"{what}: {n} bytes outside the outputs changed, arena offsets {first}..{last}; the first is in {where} "
                             f"(now {int(self.buf[first]):#x}, was {int(self.snap[first]):#x})")

    def out_bytes(self):
        """{name: a copy of the bytes of every "out" buffer} (uint8, so that NaN results compare by bits)"""
        return {s["name"]: self.buf[s["off"]:s["off"] + s["nbytes"]].clone() for s in self.specs if s["role"] == "out"}


# ---------------------------------------------------------------------------------------------------------------------------
# the three runs of tests/test_gpu_containment.py on operands given as (name, role, tensor-or-(shape, dtype))
# ---------------------------------------------------------------------------------------------------------------------------
def _spec(x):
    """(like, shape, dtype) of an operand's third field"""
    return (x, None, None) if torch.is_tensor(x) else (None, tuple(x[0]), x[1])


def run_guarded(operands, call, fill, dev, what, sync=lambda: None):
    """The call on views of one arena filled with `fill`: (status, {out name: bytes}, views).  arena.check() has passed."""
    ar = Arena(fill)
    for name, role, x in operands:
        like, shape, dtype = _spec(x)
        ar.add(name, like=like, shape=shape, dtype=dtype, role=role)
    views = dict(zip([o[0] for o in operands], ar.build(dev)))
    sync()
    status = call(views)
    sync()
    ar.check(f"{what}, fill {fill:#x}")
    return status, ar.out_bytes(), views


def run_plain(operands, call, dev, sync=lambda: None):
    """The call on ordinary separate allocations, every workspace twice as large: (status, {out name: bytes}, views)."""
    views = {}
    for name, role, x in operands:
        like, shape, dtype = _spec(x)
        if role == "ws" and like is not None:
            v = torch.cat([like.reshape(-1), like.reshape(-1)]).to(dev)
        elif role == "ws":
            nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
            v = torch.full((2 * nbytes,), PLAIN, dtype=torch.uint8, device=dev).view(dtype)
        elif like is not None:
            v = like.clone().to(dev)
        else:
            nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
            v = torch.full((nbytes,), PLAIN, dtype=torch.uint8, device=dev).view(dtype).view(shape)
        views[name] = v
    sync()
    status = call(views)
    sync()
    outs = {name: views[name].contiguous().view(-1).view(torch.uint8).clone() for name, role, _ in operands if role == "out"}
    return status, outs, views


def compare_outputs(a, b, what):
    """every output of run `a` is byte-equal to that of run `b`"""
    assert a.keys() == b.keys(), (what, sorted(a), sorted(b))
    for name in a:
        x, y = a[name], b[name]
        assert x.shape == y.shape, f"{what}: {name}: {tuple(x.shape)} against {tuple(y.shape)} bytes"
        ne = x != y
        if bool(ne.any()):
            first = int(torch.nonzero(ne)[0])
            raise AssertionError(f"{what}: output {name} differs in {int(ne.sum())} of {x.numel()} bytes, the first at byte {first} "
                                 f"({int(x[first]):#x} against {int(y[first]):#x})")
