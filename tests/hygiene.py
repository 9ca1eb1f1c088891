"""Embedding helpers of the kernel hygiene tests (tests/test_gpu_kernel_hygiene.py).

A kernel's output must be a function of the elements inside the views it was
given and of nothing else.  ``embed`` places a tensor inside one larger
allocation whose every other element holds a chosen fill (zero, all-ones NaN
bits, or 1e30), the way the models hand kernels a channel window of a wider
concat buffer whose neighbours nobody has written yet; running the same call
with different fills and comparing the output views bit for bit shows a
kernel that loads past its view, even when it masks the surplus by a multiply
with zero (Inf * 0, NaN * 0).  Output views are embedded the same way with a
canary pattern around and NaN inside, so a store outside the view
(``guards_intact``) and an element never stored (``fully_written``) show too.

Every allocation is guarded on all sides: ``rows`` whole rows above and below
the view, ``lead`` / ``tail`` channels beside it, GUARD elements before and
after a raw 1-D argument.  The guards are part of the allocation, so a stray
access lands in them and nowhere else.

ROWS: the tallest tile among the table's kernels is 16 output rows (sconv.hip
SG::TH = NW * RW = 4 * 4, xconv.hip XG::TH = 8 * 2; dcb / sdc / conv3s2 tiles
are 8 rows) plus a 7x7 kernel's halo of 3; a pixel-shuffling epilogue stores 2
output rows per tile row (32 rows).  32 guard rows cover both.
"""
import zlib

import numpy as np
import torch

from dcvc_amd import hip as K

ROWS = 32
LEAD = TAIL = 8          # keeps the 16-byte vector paths (8 bf16 / 4 fp32 channels)
GUARD = 64               # guard elements on both sides of a raw 1-D argument
CANARY_BYTE = 0xA5
FILLS = ("zero", "nan", "big")
BIG = 1e30               # finite in fp32 / bf16, >= 2^15 (raises the split range flag), Inf as fp16

_TORCH = {K.F32: torch.float32, K.BF16: torch.bfloat16}
_INT_OF = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class HygieneError(AssertionError):
    """A hygiene check failed (an AssertionError, so pytest reports it as one)."""


def fill_(t, fill):
    """Fill tensor ``t`` (any dtype) in place: "zero", "nan" (all-ones bits; an
    integer type's minimum), "big" (1e30; an integer type's maximum) or
    "canary" (CANARY_BYTE in every byte)."""
    if fill == "canary":
        t.view(torch.uint8).fill_(CANARY_BYTE)
    elif fill == "zero":
        t.zero_()
    elif t.dtype.is_floating_point:
        if fill == "nan":
            t.view(_INT_OF[t.element_size()]).fill_(-1 if t.element_size() > 1 else 255)
        elif fill == "big":
            t.fill_(BIG)
        else:
            raise ValueError(fill)
    else:
        info = torch.iinfo(t.dtype)
        t.fill_({"nan": info.min, "big": info.max}[fill])
    return t


def _bytes(t):
    return t.contiguous().view(torch.uint8)


class EmbeddedAct(K.Act):
    """An Act whose buffer is rows [rows, rows + H) of ``big`` and whose channel
    window starts at ``lead``; ``snap`` holds the allocation's bytes as built."""
    __slots__ = ("big", "snap", "rows", "lead")


def _embedded(big, rows, H, lead, C):
    a = EmbeddedAct(big[rows:rows + H], lead, C)
    a.big, a.rows, a.lead = big, rows, lead
    a.snap = _bytes(big).clone()
    return a


def embed(nchw, dtype=K.F32, lead=LEAD, tail=TAIL, rows=ROWS, fill="zero", device=None):
    """An Act holding ``nchw`` (1, C, H, W) inside one allocation of shape
    (rows + H + rows, W, lead + C + tail): Act(big[rows:rows + H]).ch(lead, C).
    Every element outside the view holds ``fill``."""
    _, C, H, W = nchw.shape
    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    big = torch.empty((rows + H + rows, W, lead + C + tail), dtype=_TORCH[dtype], device=dev)
    fill_(big, fill)
    big[rows:rows + H, :, lead:lead + C] = nchw[0].permute(1, 2, 0).to(device=dev, dtype=_TORCH[dtype])
    return _embedded(big, rows, H, lead, C)


def embed_out(C, H, W, dtype=K.F32, lead=LEAD, tail=TAIL, rows=ROWS, device=None):
    """An output view embedded like ``embed``: the canary pattern outside the
    view, NaN (all-ones bits) inside."""
    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    big = torch.empty((rows + H + rows, W, lead + C + tail), dtype=_TORCH[dtype], device=dev)
    fill_(big, "canary")
    fill_(big[rows:rows + H, :, lead:lead + C], "nan")
    return _embedded(big, rows, H, lead, C)


def embed_raw(data, fill="zero", device=None):
    """A raw-pointer argument: the 1-D tensor ``data`` (any dtype) with GUARD
    elements of ``fill`` before and after it in one allocation.  GUARD elements
    are a multiple of 16 bytes for every type, so the data keep the alignment
    of an allocation of their own.  Returns the data's slice."""
    data = data.reshape(-1)
    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    big = torch.empty(GUARD + data.numel() + GUARD, dtype=data.dtype, device=dev)
    fill_(big, fill)
    big[GUARD:GUARD + data.numel()] = data.to(dev)
    v = big[GUARD:GUARD + data.numel()]
    v._hyg = (big, _bytes(big).clone())
    return v


def embed_raw_out(n, dtype, device=None):
    """A raw-pointer output of n elements: canary guards, NaN inside (floating
    types; the canary pattern inside for integer types)."""
    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    big = torch.empty(GUARD + n + GUARD, dtype=dtype, device=dev)
    fill_(big, "canary")
    if dtype.is_floating_point:
        fill_(big[GUARD:GUARD + n], "nan")
    v = big[GUARD:GUARD + n]
    v._hyg = (big, _bytes(big).clone())
    return v


def view_of(x):
    """The torch view of an embedded object's own elements."""
    return x.t() if isinstance(x, K.Act) else x


def bits_of(x):
    """The own elements of an embedded object as a CPU integer tensor (bit patterns)."""
    t = view_of(x).contiguous()
    return t.view(_INT_OF[t.element_size()]).cpu().clone()


def outside_changes(x, view=None):
    """Number of bytes outside the view that differ from the allocation as
    built.  ``view`` = (lead, C) overrides the channel window checked (the
    self-tests declare a wider window than the one they guard)."""
    if isinstance(x, EmbeddedAct):
        es = x.big.element_size()
        lead, C = view if view is not None else (x.lead, x.C)
        diff = (_bytes(x.big) != x.snap).view(x.big.shape[0], x.big.shape[1], x.big.shape[2] * es)
        diff[x.rows:x.rows + x.H, :, lead * es:(lead + C) * es] = False
        return int(diff.sum())
    big, snap = x._hyg
    diff = _bytes(big) != snap
    es = big.element_size()
    diff[GUARD * es:(GUARD + x.numel()) * es] = False
    return int(diff.sum())


def guards_intact(x, view=None):
    """Nothing outside the view was written (compared as uint8)."""
    return outside_changes(x, view) == 0


def fully_written(x):
    """No NaN is left inside a floating-point output view."""
    t = view_of(x)
    return not t.dtype.is_floating_point or not bool(torch.isnan(t).any())


def check_guards(x, what=""):
    n = outside_changes(x)
    if n:
        raise HygieneError(f"{what}: {n} bytes outside the view were written")


def check_written(x, what=""):
    if not fully_written(x):
        t = view_of(x)
        raise HygieneError(f"{what}: {int(torch.isnan(t).sum())} elements of the view hold NaN "
                           "(never stored, or computed from memory outside a view)")


def check_same_bits(got, want, what=""):
    """Two {name: bit tensor} dicts are equal bit for bit."""
    if set(got) != set(want):
        raise HygieneError(f"{what}: outputs {sorted(got)} != {sorted(want)}")
    for k in want:
        if got[k].shape != want[k].shape or not torch.equal(got[k], want[k]):
            n = int((got[k] != want[k]).sum()) if got[k].shape == want[k].shape else -1
            raise HygieneError(f"{what}: output {k!r} differs from the clean run in {n} elements")


def seeded(key):
    """A torch generator seeded from a string (stable across runs and processes)."""
    return torch.Generator().manual_seed(zlib.crc32(key.encode()))


def poison_on_stream():
    """Fill the LDS of 512 workgroups with all-ones bytes and the VGPRs of as
    many waves as fit with all-ones bits, on the current stream."""
    K.check(K.lib().dcvc_debug_poison_lds(160 * 1024, 512, K.stream()), "poison_lds")
    K.check(K.lib().dcvc_debug_poison_vgpr(4096, K.stream()), "poison_vgpr")


ROUTED = ("conv", "conv_ffn", "dw_conv2_split", "depth_conv_split", "depthconv_block")


class Env:
    """What one run of a table entry sees: the fill of every input's
    surroundings, a cache of the entry's constants (random data, packed
    weights, references' inputs) shared by its runs, and the registry of the
    embedded inputs and outputs the run created."""

    def __init__(self, fill, cache, poison=False, device=None, dry=False):
        self.fill, self.cache, self.poison = fill, cache, poison
        self.dry = dry            # build the call and its references only: launch nothing (CPU)
        self.dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.ins, self.outs, self.refs, self.routes = [], {}, {}, []

    # ---- constants
    def const(self, key, fn):
        if key not in self.cache:
            self.cache[key] = fn()
        return self.cache[key]

    def randn(self, key, *shape, scale=1.0):
        return self.const(key, lambda: torch.randn(*shape, generator=seeded(key)) * scale)

    def rand(self, key, *shape):
        return self.const(key, lambda: torch.rand(*shape, generator=seeded(key)))

    def randint(self, key, lo, hi, *shape, dtype=torch.int64):
        return self.const(key, lambda: torch.randint(lo, hi, shape, generator=seeded(key)).to(dtype))

    def dev_const(self, key, fn):
        """A small device-resident parameter (bias, scale, table) on its own allocation."""
        return self.const("dev:" + key, lambda: fn().to(self.dev).contiguous())

    # ---- inputs
    def x(self, nchw, dtype=K.F32, lead=LEAD, tail=TAIL):
        a = embed(nchw, dtype, lead, tail, ROWS, self.fill, self.dev)
        self.ins.append(a)
        return a

    def raw(self, data):
        v = embed_raw(data, self.fill, self.dev)
        self.ins.append(v)
        return v

    def scratch(self, n, dtype):
        """Device scratch of n elements that a kernel must write before it
        reads: guarded like a raw argument, and itself holding the fill, as
        memory nobody has written would."""
        return self.raw(fill_(torch.empty(n, dtype=dtype), self.fill))

    # ---- outputs
    def y(self, name, C, H, W, dtype=K.F32, lead=LEAD, tail=TAIL, full=True):
        a = embed_out(C, H, W, dtype, lead, tail, ROWS, self.dev)
        self.outs[name] = (a, full)
        return a

    def inout(self, name, nchw, dtype=K.F32, lead=LEAD, tail=TAIL):
        """A view the kernel reads and (partly) rewrites in place: embedded as
        an input, collected as an output."""
        a = embed(nchw, dtype, lead, tail, ROWS, self.fill, self.dev)
        self.outs[name] = (a, False)
        return a

    def yraw(self, name, n, dtype, init=None):
        v = embed_raw_out(n, dtype, self.dev)
        if init is not None:
            v.copy_(init.to(self.dev))
            v._hyg = (v._hyg[0], _bytes(v._hyg[0]).clone())
        self.outs[name] = (v, init is None)
        return v

    # ---- the call
    def launch(self, fn, *a, **kw):
        """One kernel wrapper call; in a poisoned run LDS and VGPRs are filled
        with all-ones bits on the stream just before it."""
        if self.dry:
            return None
        if self.poison:
            poison_on_stream()
        r = fn(*a, **kw)
        # dcvc_last_kernel() names the instantiation for the conv families; the
        # other wrappers launch one fixed kernel per dtype / alignment path
        name = getattr(fn, "__name__", str(fn))
        self.routes.append(K.lib().dcvc_last_kernel().decode() if name in ROUTED else "dcvc_" + name)
        return r

    def ref(self, name, fn, tol=None, kind="rel"):
        """Reference of output ``name``: fn() -> fp64 / integer tensor shaped as
        the output's view ((1, C, H, W) for an Act, flat for raw).  tol None:
        exact equality; kind "rel": max |d| / max |ref| < tol; "abs": max |d| <
        tol; "rtol": |d| < tol |ref| per element; a callable: kind(got, ref) <
        tol (got as ``values`` returns it)."""
        self.refs[name] = (fn, tol, kind)

    # ---- after the call
    def collect(self, what):
        torch.cuda.synchronize() if self.dev.type == "cuda" else None
        for x in self.ins:
            check_guards(x, f"{what} input")
        out = {}
        for name, (x, full) in self.outs.items():
            check_guards(x, f"{what} output {name!r}")
            if full:
                check_written(x, f"{what} output {name!r}")
            out[name] = bits_of(x)
        return out

    def values(self, name):
        x = self.outs[name][0]
        return x.nchw().double().cpu() if isinstance(x, K.Act) else x.cpu().clone()


def check_refs(env, what):
    for name, (fn, tol, kind) in env.refs.items():
        got, ref = env.values(name), fn()
        ref = torch.as_tensor(np.asarray(ref)) if not torch.is_tensor(ref) else ref
        if tuple(got.shape) != tuple(ref.shape):
            raise HygieneError(f"{what} {name!r}: shape {tuple(got.shape)} != reference {tuple(ref.shape)}")
        if tol is None:
            same = (torch.equal(got.double(), ref.double()) if got.dtype.is_floating_point
                    else torch.equal(got, ref.to(got.dtype)))
            if not same:
                raise HygieneError(f"{what} {name!r}: {int((got.double() != ref.double()).sum())} elements differ "
                                   "from the exact reference")
            continue
        d = (got.double() - ref.double()).abs() if not callable(kind) else None
        if callable(kind):
            err = float(kind(got, ref))
        elif kind == "rel":
            err = d.max().item() / (ref.double().abs().max().item() + 1e-12)
        elif kind == "abs":
            err = d.max().item()
        elif kind == "rtol":
            err = (d / ref.double().abs().clamp_min(1e-300)).max().item()
        else:
            raise ValueError(kind)
        kind = getattr(kind, "__name__", kind)
        print(f"hygiene {what} {name}: {kind} error {err:.3e} (bound {tol:g})")
        if not err < tol:
            raise HygieneError(f"{what} {name!r}: {kind} error {err:.3e} >= {tol:g}")


def run_entry(fn, what, guard=False, deterministic=True, fills=("nan", "big")):
    """Steps 1-5 of the hygiene table for one entry (fn(env) builds and issues
    the call).  Returns the routes the clean run's launches reported."""
    cache = {}

    def once(fill, poison=False):
        env = Env(fill, cache, poison)
        tag = f"{what} [{fill}{' poisoned' if poison else ''}]"
        if guard:
            K.split_guard_arm(env.dev)
        try:
            fn(env)
            out = env.collect(tag)
            if guard and K.split_guard_tripped():
                raise HygieneError(f"{tag}: the split range guard saw a value outside the views")
        finally:
            if guard:
                K.split_guard_disarm()
        return env, out

    env0, clean = once("zero")
    check_refs(env0, what)                                     # 1

    def same(env, got, tag):
        # bit equality with the clean run; an entry declared not run-to-run
        # deterministic is held to its step-1 reference and tolerance instead
        if deterministic:
            check_same_bits(got, clean, tag)
        else:
            check_refs(env, tag)

    same(*once("zero"), f"{what} second clean run")
    for fill in fills:                                         # 2, 3, 4
        same(*once(fill), f"{what} [{fill}]")
    same(*once("zero", poison=True), f"{what} [poisoned LDS / VGPRs]")   # 5
    return env0.routes
