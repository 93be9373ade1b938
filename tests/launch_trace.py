"""Launch trace of the gradient hand-off in dan_amd/ops.py (a helper, not a test: tests/test_launch_trace_cpu.py compares what it records
with tests/golden/launch_trace.json, tests/golden/make_launch_trace_golden.py writes that file).

The hand-off (GradSlot, the gradient sinks, the side-stream weight gradients) is host logic: which library entry point an op's forward /
backward issues, with which scalars, which operands present, in which order, and what goes back to autograd.  None of that needs a kernel
to run.  For the duration of a graph this module replaces

    ops.call / ops.stream            by a recorder (nothing is launched),
    _lib.lib                         by a stub whose capability / workspace / label answers are parameters of the run,
    torch.cuda.Event / current_stream / stream     by stubs that log (the side-stream path of the weight gradients),

builds a small graph of package ops on CPU tensors of the activation dtype (torch.empty leaves them unwritten: values are never looked
at), runs forward and backward, and returns the trace:

    ["call", name, [arguments]]      integers / floats by value; pointers as None (NULL), "p" (some tensor), "main" / "side" (a stream handle)
                                     or "sink:NAME+offset" (inside a parameter's gradient sink); ConvDesc / ConvPitch / HeadLevel by field values
    ["hook", NAME]                   GRAD_READY_HOOK fired for the variable
    ["event", stream, timing] / ["wait_event", stream] / ["stream_enter" | "stream_exit", stream]       the stubbed stream API
    ["leaf", NAME, autograd's .grad as [dtype, shape] or None, was a pointer into its sink passed to any call]       after backward()
    ["keep", [number of tensors per entry kept alive for the side stream]]
    ["profile", {label: [FLOPs per launch]}, {label: [bytes per launch]}]      where the run collects them

Pointer VALUES are not recorded (the allocator reuses addresses)."""
import contextlib
import ctypes

import torch

from dan_amd import _lib, ops

ACT = _lib.ACT_DTYPE
MAIN, SIDE = 0x10000, 0x20000          # the stub streams' handles

FLAGS = ("USE_SLOTS", "USE_JUNCTION", "USE_RELU_BITS", "USE_POOL_ARG", "POOL_ONLY_TRAIN", "FUSE_FIRST_WGRAD", "HEADS_BATCHED", "WGRAD_FIRST",
         "USE_SPLITK", "KEEP_DEFORM_COL")
DEFAULTS = dict(USE_SLOTS=True, USE_JUNCTION=True, USE_RELU_BITS=True, USE_POOL_ARG=True, POOL_ONLY_TRAIN=True, FUSE_FIRST_WGRAD=True,
                HEADS_BATCHED=True, WGRAD_FIRST=False, USE_SPLITK=True, KEEP_DEFORM_COL=True, WGRAD_STREAM=True)
SCRATCH = 4096


def config(sinks=True, caps=1, scratch=0, side=False, profile=False, **flags):
    """One run's parameters.  Every OpsContext switch is given explicitly: no DANHIP_* variable reaches a trace."""
    return {"flags": dict(DEFAULTS, **flags), "sinks": bool(sinks), "caps": int(caps), "scratch": int(scratch), "side": bool(side),
            "profile": bool(profile)}


def config_key(cfg):
    off = [k for k in FLAGS if cfg["flags"][k] != DEFAULTS[k]]
    return "sinks=%d caps=%d scratch=%d side=%d profile=%d flip=%s" % (cfg["sinks"], cfg["caps"], cfg["scratch"], cfg["side"], cfg["profile"],
                                                                          ",".join(off) or "-")


def configs():
    """Every switch against the default of the others, under sinks x capability answers; the defaults under sinks x capabilities x
    split-K scratch; the side stream under sinks x WGRAD_FIRST x profiling."""
    out = [config(sinks=s, caps=c, scratch=w) for s in (0, 1) for c in (0, 1) for w in (0, SCRATCH)]
    for f in FLAGS:
        out += [config(sinks=s, caps=c, **{f: not DEFAULTS[f]}) for s in (0, 1) for c in (0, 1)]
        out.append(config(scratch=SCRATCH, **{f: not DEFAULTS[f]}))
    out += [config(sinks=s, side=True, profile=p, WGRAD_FIRST=wf) for s in (0, 1) for wf in (False, True) for p in (False, True)]
    out.append(config(profile=True))
    out.append(config(side=True, caps=0, scratch=SCRATCH))
    return out


class _StubLib(object):
    """The host-side queries ops.py makes through _lib.lib(): every answer is a parameter of the run."""

    def __init__(self, caps, scratch):
        self.caps, self.scratch = caps, scratch

    def danhip_conv2d_fwd_pool_only(self, d):
        return self.caps

    def danhip_conv2d_fwd_emits_bits(self, d, pool):
        return self.caps

    def danhip_conv2d_bwd_data_takes_bits(self, d):
        return self.caps

    def danhip_conv2d_bwd_data_first_supported(self, d):
        return self.caps

    def danhip_conv2d_fwd_concat2_supported(self, d, c1, c2):
        return self.caps

    def danhip_deform_conv_fused(self, *a):
        return self.caps

    def danhip_conv2d_workspace_bytes(self, d, which):
        return self.scratch

    def danhip_conv2d_bwd_weight_workspace_bytes(self, d):
        return self.scratch

    def danhip_deform_conv_workspace_bytes(self, N, H, W, C, kh, kw, stride, which):
        return 64 + self.scratch

    def danhip_deform_sample_bwd_workspace_bytes(self, *a):
        return 64 + self.scratch

    def danhip_conv_kernel_label(self, d, which):
        d = d._obj
        return ("conv%dx%d_s%d_%dto%d_which%d" % (d.kh, d.kw, d.stride, d.Cin, d.Cout, which)).encode()

    def danhip_conv_wgrad_kernel_label(self, d):
        d = d._obj
        return ("wgrad%dx%d_s%d_%dto%d" % (d.kh, d.kw, d.stride, d.Cin, d.Cout)).encode()


class _Stream(object):
    def __init__(self, rec, name, handle):
        self.rec, self.name, self.cuda_stream = rec, name, handle

    def wait_event(self, ev):
        self.rec.events.append(["wait_event", self.name])

    def wait_stream(self, other):
        self.rec.events.append(["wait_stream", self.name, other.name])


class Recorder(object):
    def __init__(self):
        self.events = []
        self.names = {}              # id(variable) -> name
        self.leaves = []             # (name, variable)
        self.sinks = []              # (name, first byte, one past the last byte)
        self.sink_hit = set()
        self.keep = []               # what must stay alive for the ids above to stay unique
        self.main = _Stream(self, "main", MAIN)
        self.side = _Stream(self, "side", SIDE)

    # ---- what replaces ops.call / ops.stream
    def stream(self):
        return ctypes.c_void_p(MAIN)

    def call(self, name, *args):
        if name == "danhip_conv_packed_dims":            # the one call whose OUTPUT the host uses: some non-empty packing
            d = args[0]._obj
            args[2]._obj.value, args[3]._obj.value = (d.Cout + 7) // 8 * 8, d.kh * d.kw * d.Cin
        self.events.append(["call", name, [self._arg(a) for a in args]])

    def hook(self, p):
        self.events.append(["hook", self.names[id(p)]])

    def _pointer(self, v):
        if not v:
            return None
        if v == MAIN:
            return "main"
        if v == SIDE:
            return "side"
        for name, lo, hi in self.sinks:
            if lo <= v < hi:
                self.sink_hit.add(name)
                return "sink:%s+%d" % (name, v - lo)
        return "p"

    def _struct(self, s):
        out = [type(s).__name__]
        for f, t in s._fields_:
            v = getattr(s, f)
            out.append(self._pointer(v) if t is ctypes.c_void_p else v)
        return out

    def _arg(self, a):
        if a is None:
            return None
        if isinstance(a, bool):
            return int(a)
        if isinstance(a, (int, float)):
            return a
        if isinstance(a, ctypes.c_void_p):
            return self._pointer(a.value)
        if isinstance(a, ctypes.Array):
            return [self._struct(e) for e in a]
        if isinstance(a, ctypes.Structure):
            return self._struct(a)
        o = getattr(a, "_obj", None)                     # ctypes.byref(...)
        if isinstance(o, ctypes.Structure):
            return self._struct(o)
        if o is not None:
            return "out"
        raise TypeError("launch trace: argument of type %r" % type(a).__name__)

    # ---- variables
    def act(self, *shape):
        return torch.empty(shape, dtype=ACT)

    def param(self, name, *shape, sink):
        """A trainable variable; with `sink` it carries the gradient sink a trainer's flat buffer would give it."""
        p = torch.nn.Parameter(torch.zeros(shape, dtype=torch.float32))
        if sink:
            p._danhip_grad = torch.zeros(shape, dtype=torch.float32)
            lo = p._danhip_grad.data_ptr()
            self.sinks.append((name, lo, lo + 4 * p.numel()))
        self.names[id(p)] = name
        self.leaves.append((name, p))
        self.keep.append(p)
        return p

    def finish(self, ctx):
        for name, p in self.leaves:
            g = p.grad
            self.events.append(["leaf", name, None if g is None else [str(g.dtype), list(g.shape)], name in self.sink_hit])
        self.events.append(["keep", [len(k) for k in ctx.wgrad["keep"]]])
        if ctx.PROFILE is not None:
            self.events.append(["profile", {k: [f for _, _, f in v] for k, v in sorted(ctx.PROFILE.items())},
                                {k: list(v) for k, v in sorted(ctx.PROFILE_BYTES.items())}])


@contextlib.contextmanager
def _patched(rec, cfg):
    class Event(object):
        def __init__(self, enable_timing=False):
            self.timing = bool(enable_timing)

        def record(self, st=None):
            rec.events.append(["event", st.name, int(self.timing)])

    @contextlib.contextmanager
    def stream_scope(st):
        rec.events.append(["stream_enter", st.name])
        yield
        rec.events.append(["stream_exit", st.name])

    saved = (ops.call, ops.stream, _lib.lib, torch.cuda.Event, torch.cuda.current_stream, torch.cuda.stream)
    ops.call, ops.stream = rec.call, rec.stream
    stub = _StubLib(cfg["caps"], cfg["scratch"])
    _lib.lib = lambda: stub
    torch.cuda.Event, torch.cuda.current_stream, torch.cuda.stream = Event, (lambda *a: rec.main), stream_scope
    for cache in (ops._SCRATCH_BYTES, ops._PACKED, ops._PACK_TABLE_OF):      # derived data of earlier runs (other answers, dead variables)
        cache.clear()
    try:
        yield
    finally:
        ops.call, ops.stream, _lib.lib, torch.cuda.Event, torch.cuda.current_stream, torch.cuda.stream = saved
        for cache in (ops._SCRATCH_BYTES, ops._PACKED, ops._PACK_TABLE_OF):
            cache.clear()


def _total(*ts):
    """A plain torch consumer: its gradient reaches the producers through autograd's own edges."""
    return sum(t.float().sum() for t in ts)


# ---- graph A: S3FD-shaped.  First layer (8-channel image, 3 real), conv + pool with pool_only, a tapped 64-channel map feeding both the L2
# norm and the 2 x 2 max-pool (the gradient junction), a stride-2 convolution, three head convolutions (Cout 8, 7 and 6) into heads_split.
def graph_a(rec, sinks):
    P = lambda name, *shape: rec.param(name, *shape, sink=sinks)
    img = rec.act(1, 8, 8, 8)
    y11 = ops.conv2d(img, P("conv1_1/w", 3, 3, 3, 64), P("conv1_1/b", 64), relu=True)
    y12 = ops.conv2d(y11, P("conv1_2/w", 3, 3, 64, 64), P("conv1_2/b", 64), relu=True, pool=True, pool_only=True)
    p1 = ops.max_pool_2x2(y12)
    t = ops.conv2d(p1, P("conv2_1/w", 3, 3, 64, 64), P("conv2_1/b", 64), relu=True)
    n = ops.l2_normalize(t, P("norm/gamma", 64))
    p2 = ops.max_pool_2x2(t)
    s = ops.conv2d(p2, P("conv3_1/w", 3, 3, 64, 64), P("conv3_1/b", 64), stride=2, relu=True)
    hs = [ops.conv2d(n, P("head1/w", 3, 3, 64, 8), P("head1/b", 8), out_f32=True, dy_slot=True),
          ops.conv2d(p2, P("head2/w", 3, 3, 64, 7), P("head2/b", 7), out_f32=True, dy_slot=True),
          ops.conv2d(s, P("head3/w", 3, 3, 64, 6), P("head3/b", 6), out_f32=True, dy_slot=True)]
    loc, cls = ops.heads_split(hs, [(3, 1), (2, 1), (1, 1)])
    return loc.sum() + cls.sum()


# ---- graph B: DAN-shaped.  context_block, concat of two ragged-width maps, add (ReLU operand first: one-pass residual backward; and not),
# avg_pool_2x2_s1, resize_bilinear_add with and without a lateral, concat_conv1x1_relu with split, an offset convolution (ragged Cout) into
# deform_conv, batch_norm_train and max_pool_3x3_s2 (plain autograd nodes downstream of the hand-off).
def graph_b(rec, sinks):
    P = lambda name, *shape: rec.param(name, *shape, sink=sinks)
    inp, inp2 = rec.act(1, 4, 4, 64), rec.act(1, 8, 8, 64)
    x = ops.conv2d(inp, P("stem/w", 1, 1, 64, 256), P("stem/b", 256), relu=True)
    shapes = (("b1", 1, 1, 256, 64), ("cat", 1, 1, 256, 192), ("b3plus", 3, 3, 64, 64), ("b43", 3, 3, 64, 64), ("b4plus", 3, 3, 64, 64),
              ("res", 1, 1, 256, 256))
    params = [(P("cb/%s/w" % s[0], *s[1:]), P("cb/%s/b" % s[0], s[4])) for s in shapes]
    cb = ops.context_block(x, params, [w for w, _ in reversed(params)])
    ra = ops.conv2d(inp, P("ra/w", 1, 1, 64, 85), P("ra/b", 85), relu=True)
    rb = ops.conv2d(inp, P("rb/w", 1, 1, 64, 171), P("rb/b", 171), relu=True)
    cc = ops.concat([ra, rb])
    s = ops.add(cc, cb)
    ap = ops.avg_pool_2x2_s1(s)
    s2 = ops.add(ap, s)
    up = ops.conv2d(s2, P("up/w", 1, 1, 256, 64), P("up/b", 64))
    lat = ops.conv2d(inp2, P("lat/w", 1, 1, 64, 64), P("lat/b", 64))
    m = ops.resize_bilinear_add(up, lat)
    m2 = ops.resize_bilinear_add(up, None, size=(8, 8))
    mix = ops.concat_conv1x1_relu(m2, m, P("mix/w", 1, 1, 128, 64), P("mix/b", 64), split=(64, 32))
    off = ops.conv2d(mix, P("offset/w", 3, 3, 64, 18), P("offset/b", 18))
    dc = ops.deform_conv(mix, P("deform/w", 1, 1, 9 * 64, 64), P("deform/b", 64), off, 3, 3, relu=True)
    mm, mv = torch.zeros(64), torch.ones(64)
    bn = ops.batch_norm_train(dc, P("bn/gamma", 64), P("bn/beta", 64), mm, mv, relu=True)
    return _total(ops.max_pool_3x3_s2(bn), m2)


# ---- graph C: mixed routes.  An activation with a slot is consumed by two package ops AND a plain torch op, so its producer gets slot
# deliveries and an autograd dy in the same backward: a ReLU convolution, a linear convolution, and concat's ragged-width output.  Plus a
# gradient junction in the other order than graph A's.
def graph_c(rec, sinks):
    P = lambda name, *shape: rec.param(name, *shape, sink=sinks)
    inp = rec.act(1, 4, 4, 64)
    x0 = ops.conv2d(inp, P("c0/w", 3, 3, 64, 64), P("c0/b", 64), relu=True)
    outs = []
    for tag, relu in (("relu", True), ("lin", False)):
        y = ops.conv2d(x0, P(tag + "/w", 3, 3, 64, 64), P(tag + "/b", 64), relu=relu)
        outs += [y, ops.conv2d(y, P(tag + "/a/w", 1, 1, 64, 64), P(tag + "/a/b", 64), relu=True), ops.conv2d(y, P(tag + "/b/w", 3, 3, 64, 64))]
    c64 = ops.conv2d(inp, P("c64/w", 1, 1, 64, 64), P("c64/b", 64), relu=True)
    c85 = ops.conv2d(inp, P("c85/w", 1, 1, 64, 85), P("c85/b", 85), relu=True)
    cr = ops.concat([c64, c85])                          # 149 channels: the slot carries 152
    k1 = ops.concat([cr, ops.conv2d(inp, P("c107a/w", 1, 1, 64, 107), P("c107a/b", 107))])
    k2 = ops.concat([ops.conv2d(inp, P("c107b/w", 1, 1, 64, 107), P("c107b/b", 107), relu=True), cr])
    outs += [cr, ops.conv2d(k1, P("z1/w", 1, 1, 256, 64), P("z1/b", 64)), ops.conv2d(k2, P("z2/w", 1, 1, 256, 64), P("z2/b", 64), relu=True)]
    # a second junction whose L2 norm is created after the pool, so that backward reaches it first (graph A: the pool first)
    t = ops.conv2d(inp, P("tap/w", 3, 3, 64, 64), P("tap/b", 64), relu=True)
    p = ops.max_pool_2x2(t)
    n = ops.l2_normalize(t, P("tap/gamma", 64))
    outs += [ops.conv2d(p, P("tap/p/w", 1, 1, 64, 64), P("tap/p/b", 64)), ops.conv2d(n, P("tap/n/w", 1, 1, 64, 64), P("tap/n/b", 64))]
    return _total(*outs)


GRAPHS = {"A": graph_a, "B": graph_b, "C": graph_c}


def run(graph, cfg):
    """-> the trace (a list of JSON values) of forward + backward of GRAPHS[graph] under cfg."""
    rec = Recorder()
    ctx = ops.OpsContext(**cfg["flags"])
    ctx.GRAD_READY_HOOK = rec.hook
    if cfg["profile"]:
        ctx.PROFILE, ctx.PROFILE_BYTES = {}, {}
    if cfg["side"]:                                      # what wgrad_overlap_begin() arms on a GPU
        ctx.wgrad.update(on=True, side=rec.side, main=rec.main)
    with _patched(rec, cfg), ops.use_context(ctx):
        loss = GRAPHS[graph](rec, cfg["sinks"])
        rec.events.append(["backward"])
        loss.backward()
        rec.finish(ctx)
    return rec.events


def run_all():
    """{"<graph> <configuration>": trace} over GRAPHS x configs()."""
    return {"%s %s" % (g, config_key(c)): run(g, c) for g in sorted(GRAPHS) for c in configs()}
