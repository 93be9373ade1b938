"""torch.autograd.Function wrappers over the libdanhip C ABI (device memory / streams / autograd are PyTorch
plumbing; all arithmetic happens in the HIP kernels).  Activations are NHWC 16-bit tensors (bf16, or fp16 with DANHIP_DTYPE=fp16: _lib.ACT_DTYPE).

Gradient sinks: when a parameter carries a `_danhip_grad` tensor (a view into the trainer's flat fp32 gradient
buffer) the backward kernels accumulate straight into it and return None to autograd; otherwise a fresh
gradient tensor is returned as usual (used by the parity tests with torch.autograd.grad).
"""
import contextlib
import ctypes
import os

import torch

from . import _lib
from ._lib import ACT_DTYPE as ACT, BF16, F32, SPLIT3, ConvDesc, call, ptr, stream


class OpsContext(object):
    """Everything mutable that STEERS the ops of this module, in one object (SURVEY 8b "no mutable globals on the data path"; VERDICT r4
    item 9): which kernel form an op launches, where it reports, and the per-step hooks a trainer arms.  Rounds 1-4 kept these as module
    attributes (`ops.USE_SLOTS = False` ...); those names still read and write through to the ACTIVE context (module __getattr__ /
    __setattr__ at the end of the file), so tests and A/B scripts are unchanged, but a caller can now hold its own:

        ctx = ops.OpsContext(USE_SPLITK=False)
        with ops.use_context(ctx): ...            # every op issued inside (and the backward of those ops, if run inside) sees ctx

    A DetectorTrainer keeps the context it was built under (`trainer.ops_ctx`) and runs its steps inside it.  The active context is
    process-wide, not thread-local: autograd runs backward functions on its own threads, and the deployment model is one process per GPU.
    What is NOT in here are caches (packed weights and their version stamp WEIGHT_EPOCH, scratch sizes): derived data, not steering.

    Kernel-form switches (results agree up to fp32 summation order whatever they say):
      USE_SPLITK       False: never pass the split-K scratch buffer (every shape on its single-pass kernel)
      USE_SLOTS        False: activation gradients travel through autograd's own edges instead of the direct hand-off (GradSlot), which
                       gives the parity tests a second, independent route through the same kernels (tests/test_grad_parity_gpu.py)
      USE_RELU_BITS    [DANHIP_RELU_BITS, 1]  0: ReLU masks read as 16-bit activations instead of bit masks (danhip_relu_bits: for the
                       data-gradient kernels that stage them in LDS; every consumer of an activation shares ONE holder hung on the
                       tensor, which the first backward that needs the bits fills)
      USE_POOL_ARG     [DANHIP_POOL_ARG, 1]   0: max-pool backward re-reads the activation to find each window's maximum (round 3) instead
                       of scattering through the 2-bit arg-max codes its forward kept (round 4, danhip_maxpool2x2_bwd_arg: 1.28 instead of
                       2.25 map-sized HBM passes)
      USE_JUNCTION     [DANHIP_JUNCTION, 1]   0: a map that feeds an L2 norm and a 2 x 2 max-pool gets their two gradients by two launches
                       (l2norm_bwd, then maxpool2x2_bwd_arg accumulating) instead of one danhip_l2norm_bwd_pool_scatter (dx bit-identical)
      POOL_ONLY_TRAIN  [DANHIP_POOL_ONLY_TRAIN, 1]  0: the training forward of a conv whose only consumer is a fused pool still writes its map
                       (conv1_2 / conv2_2; round 4's behaviour)
      KEEP_DEFORM_COL  False: the deformable backward re-samples the im2col buffer as the reference does instead of keeping the forward's
      WGRAD_STREAM     [DANHIP_WGRAD_STREAM, 1]  0: weight gradients on the data gradients' stream.  The environment is read ONCE, when the
                       context is made; a process that wants to switch mid-run (bench.py's serialized roofline leg, tests) assigns
                       ops.WGRAD_STREAM.  dgrad(L) and wgrad(L) both consume dY_L and are independent: on one stream each kernel's ramp-up
                       and tail (and, on the 40x40 / 20x20 maps, its under-filled grid) leave CUs idle that the other can use
                       (tools/probe_concurrent_bwd.py: conv4_2 0.95 -> 0.84 ms, conv5_1 0.37 -> 0.31, fc6 0.25 -> 0.18 for the pair)
      WGRAD_FIRST     [DANHIP_WGRAD_FIRST, 0]   1: a convolution's backward issues its weight gradient (side stream) BEFORE its data gradient, so the
                       side stream waits for dY only, not for the data gradient.  Measured slower (round 6, same box, alternating: 12.81 against
                       12.73 ms): both kernels are full-chip persistent grids, "beside each other" means taking turns, and the data gradient —
                       the critical path — then queues behind the weight gradient's workgroups
      FUSE_FIRST_WGRAD [DANHIP_FUSE_FIRST_WGRAD, 1]  0: conv1_2's data gradient stores its output and conv1_1's weight gradient is a launch of its own
                       (rounds 1-5); 1: the first layer's weight / bias gradient is folded into the second layer's data gradient
                       (danhip_conv2d_bwd_data_bits_first: conv1_1's dY never reaches HBM) where a trainer's gradient sinks exist
      HEADS_BATCHED    [DANHIP_HEADS_BATCHED, 1]  0: the detection heads split their maps (forward) and form the head convolutions' dY
                       (backward) level by level: one head_split launch per level each way plus a cast_pad launch per level, through an
                       fp32 dY, into zero-filled prediction buffers (rounds 1-11); 1: one danhip_heads_split_fwd and one
                       danhip_heads_grad_pad for all levels (heads_split; values bit-identical)
      deterministic    [DANHIP_DETERMINISTIC, 0]  True: bit-reproducible training step (the one switch that DOES change the sums' order on
                       purpose: a fixed one).  use_context sets libdanhip's option "deterministic" while this context is active; every
                       gradient / loss sum over workgroups then goes through a workspace this module allocates and the library's ordered
                       reduction (include/danhip.h "Deterministic mode") instead of float atomics, and conv1_1's weight gradient is a launch
                       of its own.  The deformable backward of DAN-Deform's shape class (3 x 3, stride 1, C / group == 64) sums its far corners in key order;
                       ops without an ordered form (other deformable shapes, batch norm, PS-ROI pooling backward) raise.  One rank only.
                       A trainer passes the flag on to FlatParams.sgd_step (the optimizer's L2 term).
      SPLIT_EVAL       True: convolutions of the fp32 inference path run as split-operand products on the fp16 MFMA (csrc/split_infer.hip;
                       models set it for precision "split"): fp32-accurate boxes at a third of the 16-bit rate instead of a tenth
    Diagnostic sinks (None = off): TRACE (tests: a dict in which every ReLU layer files its output under id(weight variable) and every
    2 x 2 max-pool its input under "pools", in call order - the discrete decisions of a forward pass, which the gradient-parity tests
    impose on the oracle graph), PROFILE / PROFILE_BYTES (bench.py: dicts; every conv forward / data-gradient / weight-gradient launch is
    bracketed by events on its stream and filed under its kernel-instance label with its algorithmic FLOPs / bytes).
    Per-step state a trainer arms: GRAD_READY_HOOK (callback(param) right after a layer's weight / bias gradients have been issued in
    backward: the data-parallel trainer launches its bucketed all-reduce from it while backward continues), LOSS_SCALE_DEV (1-element
    device tensor of the dynamic loss scale, set around the backward pass), wgrad (the second backward stream: {"on", "side", "main",
    "keep"}; switched on around the backward pass and joined before the gradients are consumed; "keep" holds the tensors the side
    stream still reads until that join: no allocator reuse while in flight, also valid inside a hipGraph capture)."""
    __slots__ = ("USE_SPLITK", "USE_SLOTS", "USE_RELU_BITS", "USE_POOL_ARG", "USE_JUNCTION", "POOL_ONLY_TRAIN", "KEEP_DEFORM_COL", "WGRAD_STREAM", "WGRAD_FIRST", "FUSE_FIRST_WGRAD", "HEADS_BATCHED", "SPLIT_EVAL", "deterministic", "TRACE",
                 "PROFILE", "PROFILE_BYTES", "GRAD_READY_HOOK", "LOSS_SCALE_DEV", "wgrad")

    def __init__(self, **overrides):
        env = os.environ.get
        self.USE_SPLITK = True
        self.USE_SLOTS = True
        self.USE_RELU_BITS = env("DANHIP_RELU_BITS", "1") == "1"
        self.USE_POOL_ARG = env("DANHIP_POOL_ARG", "1") == "1"
        self.USE_JUNCTION = env("DANHIP_JUNCTION", "1") == "1"
        self.POOL_ONLY_TRAIN = env("DANHIP_POOL_ONLY_TRAIN", "1") == "1"
        self.KEEP_DEFORM_COL = True
        self.WGRAD_STREAM = env("DANHIP_WGRAD_STREAM", "1") == "1"
        self.WGRAD_FIRST = env("DANHIP_WGRAD_FIRST", "0") == "1"
        self.FUSE_FIRST_WGRAD = env("DANHIP_FUSE_FIRST_WGRAD", "1") == "1"
        self.HEADS_BATCHED = env("DANHIP_HEADS_BATCHED", "1") == "1"
        self.SPLIT_EVAL = False
        self.deterministic = env("DANHIP_DETERMINISTIC", "0") == "1"
        self.TRACE = self.PROFILE = self.PROFILE_BYTES = None
        self.GRAD_READY_HOOK = self.LOSS_SCALE_DEV = None
        self.wgrad = {"on": False, "side": None, "main": None, "keep": []}
        for k, v in overrides.items():
            setattr(self, k, v)                       # (AttributeError for a name that is not a field)


_CTX = OpsContext()                                   # the active context (rebound by use_context only)
_CTX_FIELDS = frozenset(OpsContext.__slots__) - {"wgrad"}


def context():
    """The active OpsContext."""
    return _CTX


@contextlib.contextmanager
def use_context(ctx):
    """Make `ctx` the active context for the duration of the block (process-wide: see OpsContext)."""
    global _CTX
    prev, _CTX = _CTX, ctx
    _sync_deterministic(prev, ctx)
    try:
        yield ctx
    finally:
        _CTX = prev
        _sync_deterministic(ctx, prev)


def deterministic_context(src=None):
    """A copy of `src` (default: the active context) with OpsContext.deterministic set - what DetectorTrainer(deterministic=True) builds
    for itself, and the way to ask for the mode where a trainer's flag refuses the model: DANTrainer(DANModel(deform=True), anchors,
    ops_ctx=ops.deterministic_context())."""
    src = src if src is not None else _CTX
    ctx = OpsContext(**{k: getattr(src, k) for k in OpsContext.__slots__ if k != "wgrad"})
    ctx.deterministic = True
    return ctx


def _sync_deterministic(old, new):
    """libdanhip's launchers read the process-wide option "deterministic" once per call: it follows the active context.  (No library call,
    and no library load, while no context asks for the mode.)"""
    if bool(old.deterministic) != bool(new.deterministic):
        call("danhip_set_option", b"deterministic", 1 if new.deterministic else 0)


def _reduce_ws(M, C, dev):
    """Workspace of the _ws forms of the memory-bound kernels in deterministic mode: -> (tensor, bytes)."""
    n = int(_lib.lib().danhip_reduce_workspace_bytes(M, C))
    return torch.empty(n, dtype=torch.uint8, device=dev), n



def _desc(N, H, W, Cin, Cout, kh, kw, stride, valid=False):
    d = ConvDesc()
    d.N, d.H, d.W, d.Cin, d.Cout, d.kh, d.kw, d.stride = N, H, W, Cin, Cout, kh, kw, stride
    if valid:                       # padding='valid': no padding, floor((in - k) / s) + 1 outputs
        d.Ho, d.Wo = (H - kh) // stride + 1, (W - kw) // stride + 1
    else:                           # padding='same' (TF): ceil(in / s) outputs, padding derived by the library
        d.Ho, d.Wo = -(-H // stride), -(-W // stride)
    return d


def packed_dims(d, which):
    r, c = ctypes.c_int64(), ctypes.c_int64()
    call("danhip_conv_packed_dims", ctypes.byref(d), which, ctypes.byref(r), ctypes.byref(c))
    return r.value, c.value


def pack_conv_weight(d, w_hwio, need_bwd=True):
    """fp32 HWIO [kh,kw,cin_real,Cout] -> (wf bf16 [Cout_pad,Kpad], wb bf16 [Cin_pad,Kpad_b] or None)."""
    assert w_hwio.dtype == torch.float32 and w_hwio.is_contiguous()
    rf, cf = packed_dims(d, 0)
    wf = torch.empty((rf, cf), dtype=ACT, device=w_hwio.device)
    wb = None
    if need_bwd:
        rb, cb = packed_dims(d, 1)
        wb = torch.empty((rb, cb), dtype=ACT, device=w_hwio.device)
    call("danhip_pack_conv_weight", ctypes.byref(d), ptr(w_hwio), w_hwio.shape[2], ptr(wf), ptr(wb), stream())
    return wf, wb


# ---- packed-weight cache.  A conv weight that is an nn.Parameter keeps its two bf16 packings in persistent buffers; they are
# reused while the parameter is unchanged (inference: no packing at all) and refreshed for ALL parameters by one launch
# after an optimizer update (repack_all).  "Unchanged" = same WEIGHT_EPOCH (bumped by the fused optimizer, which writes
# through raw pointers), same tensor version (in-place torch ops) and same storage.
WEIGHT_EPOCH = 0
_PACKED = {}
_PACK_TABLE_OF = {}          # key -> (entries, device table, workgroups, parameter ids, parameter pointers): repack_all(key, select);
                             # cleared whenever the set of cached packings or one of their buffers changes


class _Packed(object):
    __slots__ = ("ref", "key", "d", "wf", "wb", "stamp")


def _stamp(p):
    return (WEIGHT_EPOCH, p._version, p.data_ptr())


def _drop_packed(pid):
    _PACKED.pop(pid, None)
    _PACK_TABLE_OF.clear()


def packed_weights(d, w, w_param, need_bwd):
    """-> (wf, wb) for conv descriptor d; cached per Parameter, packed on the spot for plain tensors."""
    if w_param is None:
        return pack_conv_weight(d, w.detach(), need_bwd=need_bwd)
    import weakref
    key = (d.kh, d.kw, d.Cin, d.Cout, w.shape[2])
    pid = id(w_param)
    e = _PACKED.get(pid)
    if e is None or e.key != key or e.ref() is not w_param:
        e = _Packed()
        e.ref = weakref.ref(w_param, lambda _r, pid=pid: _drop_packed(pid))
        e.key, e.stamp, e.wb = key, None, None
        e.d = _desc(1, 8, 8, d.Cin, d.Cout, d.kh, d.kw, 1)           # packing depends on the kernel / channel dims only
        rf, cf = packed_dims(e.d, 0)
        e.wf = torch.empty((rf, cf), dtype=ACT, device=w.device)
        _PACKED[pid] = e
        _PACK_TABLE_OF.clear()
    if need_bwd and e.wb is None:
        rb, cb = packed_dims(e.d, 1)
        e.wb = torch.empty((rb, cb), dtype=ACT, device=w.device)
        e.stamp = None
        _PACK_TABLE_OF.clear()
    st = _stamp(w_param)
    if e.stamp != st:
        wd = w_param.detach()
        if not (wd.dtype == torch.float32 and wd.is_contiguous()):
            # e.g. a member of a fused block (VariableStore.fuse: a strided view of one flat-buffer segment once a trainer has laid the
            # block out) reached an UNFUSED convolution: the fused / unfused choice (net.danet FUSED_CONTEXT_BLOCK / FUSED_STAGE2_MIX,
            # DANHIP_FUSED_CONTEXT / DANHIP_FUSED_STAGE2_MIX) is per call, the layout is fixed when the trainer is built
            raise RuntimeError("packed_weights: a kernel variable of shape %s arrives as a non-contiguous view (strides %s): it is a member of a "
                               "fused parameter block, which only the fused op consumes - set the fused / unfused switches BEFORE the "
                               "trainer (FlatParams) is built, not between calls" % (tuple(wd.shape), tuple(wd.stride())))
        call("danhip_pack_conv_weight", ctypes.byref(e.d), ptr(wd), wd.shape[2], ptr(e.wf), ptr(e.wb), stream())
        e.stamp = st
    return e.wf, (e.wb if need_bwd else None)


def repack_all(key=None, select=None):
    """One launch refreshing every cached packing (call after the optimizer changed the parameters).
    key / select (round 5): a NAMED SUBSET of the cached packings - select(parameter) -> bool - with its own device table, for an optimizer
    that runs bucket by bucket while backward is still producing the other buckets' gradients (trainer.DetectorTrainer._bucket_opt)."""
    entries = [(e, e.ref()) for e in _PACKED.values()]
    entries = [(e, p) for e, p in entries if p is not None and (select is None or select(p))]
    if not entries:
        return
    tabs = _PACK_TABLE_OF
    tab = tabs.get(key)
    ids, ptrs = [id(p) for _, p in entries], [p.data_ptr() for _, p in entries]
    if tab is None or tab[3] != ids or tab[4] != ptrs:
        arr = (_lib.PackEntry * len(entries))()
        first = 0
        nb = ctypes.c_int32()
        for i, (e, p) in enumerate(entries):
            call("danhip_pack_entry_init", ctypes.byref(arr[i]), ctypes.byref(e.d), ptr(p.detach()), p.shape[2], ptr(e.wf), ptr(e.wb), first,
                 ctypes.byref(nb))
            first += nb.value
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        tab = tabs[key] = (len(entries), host.to(entries[0][1].device), first, ids, ptrs)
    n, dev_tab, blocks, _, _ = tab
    call("danhip_pack_conv_weights_batched", ptr(dev_tab), n, blocks, stream())
    for e, p in entries:
        e.stamp = _stamp(p)


def _grad_sink(p):
    return getattr(p, "_danhip_grad", None)


def _sink_trainable(t):
    """A fused block (not a leaf itself) whose member parameters are being trained."""
    ms = getattr(t, "_danhip_members", None)
    return ms is not None and any(m.requires_grad for m in ms)


# ---- optional per-kernel timing (OpsContext.PROFILE / PROFILE_BYTES)
def _prof_begin(st=None):
    if _CTX.PROFILE is None:
        return None
    e = torch.cuda.Event(enable_timing=True)
    e.record(st if st is not None else torch.cuda.current_stream())
    return e


def _prof_end(e0, d, which, st=None, wrote_y=True, pooled=False):
    """wrote_y = False: a pool-only launch (the full-resolution map is never stored); pooled: the launch also stores the 2x2-pooled map.
    Both only change the ALGORITHMIC byte count of the launch (conv1_2 / conv2_2 were credited the 839 / 419 MB map
    they no longer write, which filed an MFMA-bound launch under the HBM-bound ones)."""
    if e0 is None:
        return
    e1 = torch.cuda.Event(enable_timing=True)
    e1.record(st if st is not None else torch.cuda.current_stream())
    if which == 2:
        label = _lib.lib().danhip_conv_wgrad_kernel_label(ctypes.byref(d)).decode()
    else:
        label = _lib.lib().danhip_conv_kernel_label(ctypes.byref(d), which).decode()
    cin = d.Cin                              # MACs are the same for fwd and dgrad: Ho*Wo*Cin*Cout*kh*kw per image
    flops = 2.0 * d.N * d.Ho * d.Wo * cin * d.Cout * d.kh * d.kw
    _CTX.PROFILE.setdefault(label, []).append((e0, e1, flops))
    if _CTX.PROFILE_BYTES is not None:            # algorithmic HBM bytes: activations in + out (16-bit; the heads write fp32), weights once
        co8 = (d.Cout + 7) // 8 * 8
        out_px = (d.Ho * d.Wo if wrote_y else 0) + (((d.Ho + 1) // 2) * ((d.Wo + 1) // 2) if pooled else 0)
        nbytes = 2.0 * d.N * (d.H * d.W * cin + out_px * co8) + 2.0 * d.kh * d.kw * cin * d.Cout
        _CTX.PROFILE_BYTES.setdefault(label, []).append(nbytes)


# ---- weight gradients on a second stream (OpsContext.WGRAD_STREAM / wgrad)
def wgrad_overlap_begin():
    if not torch.cuda.is_available():
        return
    if not _CTX.WGRAD_STREAM:
        return
    if _CTX.wgrad["side"] is None:
        _CTX.wgrad["side"] = torch.cuda.Stream()
    _CTX.wgrad["main"] = torch.cuda.current_stream()
    _CTX.wgrad["on"] = True


def wgrad_overlap_join():
    """The launching stream waits for every weight gradient issued on the side stream; releases the kept tensors."""
    if _CTX.wgrad["on"]:
        torch.cuda.current_stream().wait_stream(_CTX.wgrad["side"])
    _CTX.wgrad["on"] = False
    _CTX.wgrad["keep"].clear()


def wgrad_streams():
    """Streams gradient producers may be running on (the data-parallel buckets wait for all of them)."""
    return [_CTX.wgrad["main"], _CTX.wgrad["side"]] if _CTX.wgrad["on"] else []



class GradSlot(object):
    """Direct gradient hand-off between this package's ops, bypassing autograd's per-edge tensors.

    Every activation produced here carries a slot.  In backward, a consumer that knows the slot writes (first delivery)
    or accumulates (later deliveries) its input-gradient contribution straight into the slot's buffer — already
    multiplied by (x > 0) when x is a ReLU output, which folds the producer's ReLU backward into the consumer's
    epilogue — and returns None to autograd.  The producer's backward then takes the buffer.  Consumers that do not
    know about slots (plain torch ops) still work: their gradient arrives through autograd and is merged in.

    An op's wrapper makes the slot UNBOUND (_new_slot), hands it to the autograd function, which keeps it for its backward, and binds it
    to the output once that exists (_publish); GradSlot(t, is_relu, channels) makes and binds in one step."""

    __slots__ = ("shape", "dtype", "device", "is_relu", "buf", "count", "taps", "pending")

    def __init__(self, t=None, is_relu=False, channels=None):
        self.buf, self.count = None, 0
        self.taps, self.pending = 0, None                # gradient junction (USE_JUNCTION): see defer()
        if t is not None:
            self.bind(t, is_relu, channels)

    def bind(self, t, is_relu, channels=None, dtype=None):
        """The buffer is a gradient of t: its shape, dtype and device - except `channels` (ragged Cout: the buffer carries the
        channel-padded gradient layout) and `dtype` (a head convolution's slot holds the 16-bit dY of its fp32 output)."""
        self.shape, self.dtype, self.device, self.is_relu = t.shape, (t.dtype if dtype is None else dtype), t.device, is_relu
        if channels is not None:
            self.shape = tuple(t.shape[:-1]) + (channels,)

    def defer(self, kind, alone, payload):
        """A delivery of a gradient junction (kind: TAP_L2NORM / TAP_POOL) takes its turn - buffer and accumulate flag exactly as
        target() hands them out - but is not launched yet: the partner's backward, if it is the next delivery, pops it and launches
        both as one kernel.  Any other delivery, or the producer's take(), first launches it on its own (`alone(buffer, acc)`), so
        the order of the roundings in the buffer never changes."""
        buf, acc = self.target()
        self.pending = (kind, acc, alone, payload)

    def pop_pending(self, kind):
        """-> (acc, payload) of the deferred delivery if it is of this kind (it is then the caller's to launch), else None."""
        p = self.pending
        if p is None or p[0] != kind:
            return None
        self.pending = None
        return p[1], p[3]

    def flush(self):
        p, self.pending = self.pending, None
        if p is not None:
            p[2](self.buf, p[1])

    def target(self):
        """-> (buffer, accumulate flag) for the next delivery."""
        self.flush()
        if self.buf is None:
            self.buf = torch.empty(self.shape, dtype=self.dtype, device=self.device)
            self.count = 0
        acc = 1 if self.count > 0 else 0
        self.count += 1
        return self.buf, acc

    def take(self):
        self.flush()
        b, n = self.buf, self.count
        self.buf, self.count = None, 0
        return b if n > 0 else None


TAP_L2NORM, TAP_POOL = 1, 2      # GradSlot.taps: the consumers of a gradient junction, registered by their forward passes


def _junction_ok(slot, dy, C):
    """May this backward node of a tapped map (it receives no raw autograd gradient: dy) defer to / fuse with its partner?"""
    return _CTX.USE_JUNCTION and slot.taps == (TAP_L2NORM | TAP_POOL) and dy is None and C in (64, 128, 256, 512)


def _slot_of(t):
    return getattr(t, "_dh_slot", None) if _CTX.USE_SLOTS else None


def _new_slot(track):
    return GradSlot() if (track and _CTX.USE_SLOTS) else None


# ---- the hand-off protocol, once.  Forward: the wrapper makes an unbound slot, the autograd function keeps it, _publish binds it to the
# output.  Backward: _incoming gathers the output gradient, _deliver hands the input gradient to the producer's slot or to autograd,
# _grad_target picks a parameter's gradient sink or a fresh tensor for autograd, _launch_wgrad issues a weight gradient on its stream.
def _pad8(c):
    return (c + 7) // 8 * 8


def _ragged(c):
    """The channel-padded width the slot of a c-wide output carries, None when c needs no padding."""
    return None if c % 8 == 0 else _pad8(c)


def _publish(y, slot, is_relu, channels=None, dtype=None):
    """Binds the slot (or None) to the output y and hangs it on the tensor, where y's consumers find it: `_dh_slot`; `_dh_pslot` when
    the buffer is channel-padded (`channels`: only ops.concat knows that layout, a ragged tensor feeds no conv directly); `_dh_hslot`
    for a head convolution, whose buffer is the 16-bit dY (`dtype`, `channels`), not a gradient of y's own type and width.  -> y"""
    if slot is not None:
        slot.bind(y, is_relu, channels, dtype)
        if dtype is not None:
            y._dh_hslot = slot
        elif channels is not None:
            y._dh_pslot = slot
        else:
            y._dh_slot = slot
    return y


def _incoming(slot, dy, prepare=None, ragged=False):
    """-> the output gradient of a backward node, or None when none reached it: what the consumers delivered into its slot (already
    ReLU-masked where the output is a ReLU's) merged with autograd's dy.  prepare(dy): a producer that must cast, pad or mask the raw
    autograd gradient first returns a contiguous tensor of its own.  dy is ADDED INTO THE SLOT'S BUFFER, never the other way round: the
    incoming tensor may be shared with other consumers.  ragged: the buffer may be channel-padded and wider than dy (ops.concat)."""
    g = slot.take() if slot is not None else None
    if dy is not None:
        if prepare is not None:
            dy = prepare(dy)
        if g is None:
            g = dy.contiguous()
        elif ragged and g.shape[-1] != dy.shape[-1]:
            g[..., :dy.shape[-1]].add_(dy)
        else:
            g.add_(dy)
    return g


def _deliver(slot, shape, like, launch):
    """The input gradient of a backward node goes straight into the producer's slot (launch(buffer, accumulate flag); -> None for
    autograd) or, without a slot, into a fresh tensor of `shape` and `like`'s type that autograd gets (launch(tensor, 0); -> it)."""
    if slot is not None:
        launch(*slot.target())
        return None
    dx = like.new_empty(shape)
    launch(dx, 0)
    return dx


def _param_handle(t):
    """t itself when it is a variable with state of its own here (cached packings, a gradient sink): an nn.Parameter, or a plain tensor
    carrying a gradient sink - a fused block of parameters (FlatParams); else None."""
    return t if (isinstance(t, torch.nn.Parameter) or hasattr(t, "_danhip_grad")) else None


def _grad_target(p, shape, device):
    """-> (fp32 tensor the kernels accumulate a parameter's gradient into, what autograd gets back): the gradient sink of handle p and
    None, or a fresh zero tensor twice."""
    sink = _grad_sink(p) if p is not None else None
    if sink is not None:
        return sink, None
    z = torch.zeros(shape, dtype=torch.float32, device=device)
    return z, z


def _launch_wgrad(d, on_side, issue, keep):
    """Issues a weight gradient of descriptor d - issue(stream handle) makes the library call - with its profiling bracket (d = None: a call
    without a conv descriptor, no bracket).  on_side and
    the trainer's second stream on: on that stream, ordered behind everything issued so far on the current one (dY is final there, and
    the sinks are zeroed), with explicit stream handles (no stream-context switch per layer on the host) and `keep` (what the call
    reads) alive until the join.  -> went to the side stream"""
    if on_side and _CTX.wgrad["on"]:
        side = _CTX.wgrad["side"]
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        side.wait_event(ev)
        e0 = _prof_begin(side) if d is not None else None
        issue(ctypes.c_void_p(side.cuda_stream))
        _prof_end(e0, d, 2, side)
        _CTX.wgrad["keep"].append(keep)
        return True
    e0 = _prof_begin() if d is not None else None
    issue(stream())
    _prof_end(e0, d, 2)
    return False


# ---- ReLU masks as bits (OpsContext.USE_RELU_BITS): one holder per activation, shared by all its consumers
def _bits_holder(x):
    h = getattr(x, "_dh_bits", None)
    if h is None:
        h = [None]
        x._dh_bits = h
    return h


def relu_bits(x, holder):
    if holder[0] is None:
        C = x.shape[-1]
        M = x.numel() // C
        b = torch.empty((M, C // 8), dtype=torch.uint8, device=x.device)
        call("danhip_relu_bits", ptr(x), ptr(b), M, C, stream())
        holder[0] = b
    return holder[0]



def _conv_scratch(d, which, dev):
    """Scratch buffer for a split-K launch of this forward (which = 0) / data-gradient (which = 1) call, or (None, 0): maps with too few
    output tiles to fill the chip (danhip_conv2d_workspace_bytes).  Only small problems are worth asking the library about."""
    M, co = (d.N * d.Ho * d.Wo, d.Cout) if which == 0 else (d.N * d.H * d.W, d.Cin)
    if not _CTX.USE_SPLITK or -(-M // 128) * -(-co // 128) > 160:
        return None, 0
    key = (which, d.N, d.H, d.W, d.Cin, d.Cout, d.kh, d.kw, d.stride, d.Ho)
    n = _SCRATCH_BYTES.get(key)
    if n is None:
        n = _SCRATCH_BYTES[key] = _lib.lib().danhip_conv2d_workspace_bytes(ctypes.byref(d), which)
    return (torch.empty(n, dtype=torch.uint8, device=dev), n) if n else (None, 0)


_SCRATCH_BYTES = {}          # (which, descriptor) -> bytes: one library query per shape (host time matters at 2 images per GPU)


def _wgrad_scratch(d, dev):
    key = (3 if _CTX.deterministic else 2, d.N, d.H, d.W, d.Cin, d.Cout, d.kh, d.kw, d.stride, d.Ho)      # (the mode changes the answer)
    n = _SCRATCH_BYTES.get(key)
    if n is None:
        n = _SCRATCH_BYTES[key] = _lib.lib().danhip_conv2d_bwd_weight_workspace_bytes(ctypes.byref(d))
    return (torch.empty(n, dtype=torch.uint8, device=dev), n) if n else (None, 0)


def _pool_arg_buffer(pooled, need_bwd):
    if not (_CTX.USE_POOL_ARG and need_bwd):
        return None
    c = pooled.shape[-1]
    return torch.empty((pooled.numel() // c, c // 4), dtype=torch.uint8, device=pooled.device)


class _Conv2d(torch.autograd.Function):
    """y = act(conv2d_same(x, w) + b) [+ residual]; tf.layers.conv2d semantics (net/sfd_net.py:81-89)."""

    @staticmethod
    def forward(ctx, x, w, b, stride, relu, out_f32, residual, w_param, b_param, xslot, yslot, pool_out=None, valid=False, block_grads=0, xbits=None, bits_out=None,
                pool_only=False, tracked=True, first=None):
        N, H, W, C = x.shape
        kh, kw, cin_real, cout = w.shape
        ctx.first = first                                # (image, kernel, bias, real channels) of the FIRST layer when x is its output (conv2d)
        assert x.dtype == ACT and x.is_contiguous(), "conv input must be contiguous NHWC bf16"
        assert C % 8 == 0 and cin_real <= C
        d = _desc(N, H, W, C, cout, kh, kw, stride, valid)
        need_bwd = w.requires_grad or x.requires_grad or bool(block_grads)
        wf, wb = packed_weights(d, w, w_param, need_bwd)
        if pool_only == 1 and pool_out is not None and _lib.lib().danhip_conv2d_fwd_pool_only(ctypes.byref(d)):      # (nothing is tracked)
            # inference: nothing but the pool reads this activation - the kernel pools in its epilogue and never writes the full-resolution map
            pooled = torch.empty((N, (d.Ho + 1) // 2, (d.Wo + 1) // 2, cout), dtype=ACT, device=x.device)
            e0 = _prof_begin()
            call("danhip_conv2d_fwd_pool", ctypes.byref(d), ptr(x), ptr(wf), ptr(b.detach()), None, ptr(pooled), stream())
            _prof_end(e0, d, 4, wrote_y=False, pooled=True)
            pooled._dh_already_pooled = True
            return pooled
        # pool_only == 2 (training): nothing but the fused pool reads this activation, and backward reaches it only through the pool's arg-max
        # codes and the pooled map's sign (the gradient arrives already masked in the slot) - the kernel gets y = NULL and skips the
        # full-resolution stores (conv1_2: 839 MB, conv2_2: 419 MB per batch of 16 at 640 x 640).  The tensor autograd sees is a
        # zero-stride view of one element: any op that tried to READ it fails ptr()'s contiguity assertion instead of reading garbage.
        skip_y = (pool_only == 2 and pool_out is not None and _CTX.USE_POOL_ARG and need_bwd and b is not None
                  and bool(_lib.lib().danhip_conv2d_fwd_pool_only(ctypes.byref(d)))
                  and _conv_scratch(d, 0, x.device)[1] == 0)          # (a map small enough to split K runs the pool as its own kernel)
        if skip_y:
            y = torch.empty((1,), dtype=ACT, device=x.device).expand(N, d.Ho, d.Wo, cout)
        else:
            y = torch.empty((N, d.Ho, d.Wo, cout), dtype=torch.float32 if out_f32 else ACT, device=x.device)
        yp = None if skip_y else ptr(y)
        e0 = _prof_begin()
        emit = (bits_out is not None and relu and not out_f32 and residual is None and b is not None
                and _lib.lib().danhip_conv2d_fwd_emits_bits(ctypes.byref(d), 1 if pool_out is not None else 0))
        if emit:                                         # conv_relu (+ fused pool) that also leaves the ReLU bit masks for the next conv's data gradient
            ybits = torch.empty((N * d.Ho * d.Wo, cout // 8), dtype=torch.uint8, device=x.device)
            pooled = pbits = parg = None
            if pool_out is not None:
                pooled = torch.empty((N, (d.Ho + 1) // 2, (d.Wo + 1) // 2, cout), dtype=ACT, device=x.device)
                pbits = torch.empty((pooled.numel() // cout, cout // 8), dtype=torch.uint8, device=x.device)
                parg = _pool_arg_buffer(pooled, need_bwd and tracked)
                pool_out.extend([pooled, parg])
            call("danhip_conv2d_fwd_relu_bits_arg", ctypes.byref(d), ptr(x), ptr(wf), ptr(b.detach()), yp, ptr(ybits), ptr(pooled), ptr(pbits), ptr(parg),
                 stream())
            bits_out.extend([ybits, pbits])
        elif pool_out is not None:                       # conv_relu + the block's 2x2 max-pool in one call (fused epilogue where possible)
            assert relu and not out_f32 and residual is None and b is not None and cout % 8 == 0
            pooled = torch.empty((N, (d.Ho + 1) // 2, (d.Wo + 1) // 2, cout), dtype=ACT, device=x.device)
            parg = _pool_arg_buffer(pooled, need_bwd and tracked)
            ws, nws = _conv_scratch(d, 0, x.device)
            if nws:                                      # a map small enough to split K: no kernel of it fuses the pool anyway
                assert not skip_y
                call("danhip_conv2d_fwd_ws", ctypes.byref(d), ptr(x), ptr(wf), ptr(b.detach()), ptr(y), BF16, 1, None, ptr(ws), nws, stream())
                call("danhip_maxpool2x2_fwd_arg", ptr(y), ptr(pooled), ptr(parg), N, d.Ho, d.Wo, cout, stream())
            else:
                call("danhip_conv2d_fwd_pool_arg", ctypes.byref(d), ptr(x), ptr(wf), ptr(b.detach()), yp, ptr(pooled), ptr(parg), stream())
            pool_out.extend([pooled, parg])
        else:
            ws, nws = _conv_scratch(d, 0, x.device)
            call("danhip_conv2d_fwd_ws", ctypes.byref(d), ptr(x), ptr(wf), ptr(b.detach()) if b is not None else None, ptr(y),
                 F32 if out_f32 else BF16, int(relu), ptr(residual), ptr(ws), nws, stream())
        _prof_end(e0, d, 4 if pool_out is not None else 0, wrote_y=not skip_y, pooled=pool_out is not None)
        ctx.d, ctx.relu, ctx.cin_real = d, relu, cin_real
        ctx.out_f32 = out_f32
        ctx.xslot, ctx.yslot, ctx.xbits = xslot, yslot, xbits
        ctx.set_materialize_grads(False)
        ctx.has_res = residual is not None
        ctx.w_param, ctx.b_param = w_param, b_param
        ctx.save_for_backward(x, wb, y if (relu and not skip_y) else None)
        ctx.y_unwritten = skip_y
        ctx.has_bias = b is not None
        ctx.block_w, ctx.block_b = bool(block_grads & 1), bool(block_grads & 2)   # fused parameter blocks: not autograd leaves themselves
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wb, y = ctx.saved_tensors
        d = ctx.d
        co8 = (d.Cout + 7) // 8 * 8
        M = d.N * d.Ho * d.Wo
        wp, bp = ctx.w_param, ctx.b_param
        need_dw = ctx.needs_input_grad[1] or ctx.block_w
        need_db = ctx.has_bias and (ctx.needs_input_grad[2] or ctx.block_b)
        db, db_ret = _grad_target(bp, (d.Cout,), x.device) if need_db else (None, None)
        if dy is not None and ctx.y_unwritten:
            raise RuntimeError("conv2d(pool_only=True): the full-resolution activation was never written, but a gradient reached it outside the "
                               "fused pool's direct hand-off (some op other than max_pool_2x2 consumed it)")
        dres = dy if ctx.has_res else None               # residual is added after the activation

        def prepare(dy):                                 # the autograd tensor: to the slot's layout, times this layer's own ReLU mask
            if dy.dtype != ACT or dy.shape[-1] != co8:
                # fp32 / unpadded upstream gradient (head convs): cast + pad channels to a multiple of 8
                src = dy.contiguous().to(torch.float32)
                dyp = torch.empty((d.N, d.Ho, d.Wo, co8), dtype=ACT, device=dy.device)
                # ragged Cout: y has Cout (not co8) channels per row, so its ReLU mask is applied here, on the unpadded layout
                call("danhip_cast_pad_f32_to_bf16", ptr(src), ptr(y) if (ctx.relu and d.Cout != co8) else None, ptr(dyp), M, d.Cout, co8, stream())
                dy, owned = dyp, True
                masked = ctx.relu and d.Cout != co8
            else:
                dy, owned = dy.contiguous(), False
                masked = False
            if ctx.relu and not masked:
                if not owned:
                    dy = dy.clone()                      # the incoming gradient tensor may be shared with other consumers
                call("danhip_relu_bwd_bias_grad", ptr(dy), ptr(y), None, M, co8, stream())
            return dy

        g = _incoming(ctx.yslot, dy, prepare)            # slot deliveries (already ReLU-masked) and / or the autograd tensor
        if g is None:                                    # no gradient reached this layer
            return (None,) * 19
        if _CTX.TRACE is not None and ctx.out_f32:       # tests: the 16-bit dY of every head convolution, in backward order
            _CTX.TRACE.setdefault("head_dy", []).append(g)
        db_in_wgrad = need_db and need_dw                        # the weight-gradient kernel also emits the bias gradient
        if need_db and not db_in_wgrad:
            if co8 == d.Cout and _CTX.deterministic:
                rws, nrws = _reduce_ws(M, co8, g.device)
                call("danhip_relu_bwd_bias_grad_ws", ptr(g), None, ptr(db), M, co8, ptr(rws), nrws, stream())
            elif co8 == d.Cout:
                call("danhip_relu_bwd_bias_grad", ptr(g), None, ptr(db), M, co8, stream())
            else:
                db.add_(g.view(M, co8)[:, :d.Cout].to(torch.float32).sum(0))
        # Order of the two launches (ops.WGRAD_FIRST, round 6).  Default: data gradient first — the side stream's event is recorded BEHIND it, so
        # wgrad(L) waits for dgrad(L) to finish and runs beside dgrad(L-1); at the end of backward conv1_2's weight gradient (0.44 ms) and conv1_1's
        # (0.19 ms) run with the other queue empty (profiles/r5/s3fd_b16_step_timeline_full.txt: VERDICT r5's "0.63 ms single-queue tail").
        # WGRAD_FIRST issues the weight gradient first (its event then waits for dY only).  Measured on one box, alternating processes
        # (profiles/r6/ab_wgrad_first_same_box.txt): 12.81 ms against 12.73 for the default — SLOWER.  Two full-chip persistent grids cannot share
        # a CU, so "beside" means taking turns: what the second queue buys is tail filling, whatever the order, and with the weight gradient
        # ahead the data-gradient chain (the critical path: every later layer waits for it) queues behind 256 weight-gradient workgroups.  The
        # tail cannot be closed by reordering: conv1_2's two gradients are both chip-filling and conv1_1's needs conv1_2's data gradient.
        dx = None
        dw = None
        hooked = False
        fused_first = False

        def launch_dx():
            nonlocal dx, fused_first
            if ctx.needs_input_grad[0]:
                xs = ctx.xslot
                fi = ctx.first
                if (fi is not None and _CTX.FUSE_FIRST_WGRAD and xs is not None and xs.is_relu and xs.count == 0 and ctx.xbits is not None
                        and _grad_sink(fi[1]) is not None and (fi[2] is None or _grad_sink(fi[2]) is not None)
                        and _lib.lib().danhip_conv2d_bwd_data_first_supported(ctypes.byref(d))):
                    # x is the FIRST layer's output: that layer has no data gradient, so this call's dX would be read by nothing but its weight
                    # gradient — the kernel folds that product in (dX tile in LDS x image patch), adds it to the first layer's gradient sinks and
                    # never stores dX; the slot stays empty and the first layer's backward finds nothing to do
                    e0 = _prof_begin()
                    call("danhip_conv2d_bwd_data_bits_first", ctypes.byref(d), ptr(g), ptr(wb), ptr(relu_bits(x, ctx.xbits)), ptr(fi[0]), int(fi[3]),
                         ptr(_grad_sink(fi[1])), ptr(_grad_sink(fi[2])) if fi[2] is not None else None, stream())
                    _prof_end(e0, d, 5, wrote_y=False)       # (dX is never stored: algorithmic bytes = dY + bit mask + image + weights)
                    fused_first = True
                    return
                relu_x = xs is not None and xs.is_relu

                def data_grad(buf, acc):                     # into the producer's slot (+ its ReLU backward), or a tensor for autograd
                    e0 = _prof_begin()
                    if relu_x and ctx.xbits is not None and _lib.lib().danhip_conv2d_bwd_data_takes_bits(ctypes.byref(d)):
                        # the kernel keeps its tile's mask in LDS as bits: 1/16 of the bytes, and not a load in its epilogue
                        call("danhip_conv2d_bwd_data_bits", ctypes.byref(d), ptr(g), ptr(wb), ptr(relu_bits(x, ctx.xbits)), ptr(buf), acc, stream())
                    else:
                        ws, nws = _conv_scratch(d, 1, g.device)
                        call("danhip_conv2d_bwd_data_ws", ctypes.byref(d), ptr(g), ptr(wb), ptr(x) if relu_x else None, ptr(buf), acc, ptr(ws), nws,
                             stream())
                    _prof_end(e0, d, 5 if relu_x else 1)

                dx = _deliver(xs, x.shape, x, data_grad)

        def launch_dw():
            nonlocal dw, hooked
            if need_dw:
                dw_to, dw = _grad_target(wp, (d.kh, d.kw, ctx.cin_real, d.Cout), g.device)
                # split partial sums as plain stores into a scratch slab + a combine pass, where the library's kernel for this shape offers it
                ws, nws = _wgrad_scratch(d, g.device)

                def issue(st):
                    call("danhip_conv2d_bwd_weight_ws", ctypes.byref(d), ptr(x), ptr(g), ptr(dw_to), ptr(db) if db_in_wgrad else None, ctx.cin_real,
                         ptr(ws), nws, st)

                # (the side stream only with a gradient sink: a gradient handed back to autograd is consumed on this stream)
                if _launch_wgrad(d, dw is None, issue, (g, x, ws)):
                    if _CTX.GRAD_READY_HOOK is not None and wp is not None:
                        _CTX.GRAD_READY_HOOK(wp)                 # the buckets wait for both gradient streams (trainer.GradBuckets._launch_ready)
                    hooked = True

        if _CTX.WGRAD_FIRST:
            launch_dw()
            launch_dx()
        else:
            launch_dx()
            launch_dw()
        if _CTX.GRAD_READY_HOOK is not None and wp is not None and not hooked:
            _CTX.GRAD_READY_HOOK(wp)
        if fused_first and _CTX.GRAD_READY_HOOK is not None:
            _CTX.GRAD_READY_HOOK(ctx.first[1])           # the first layer's gradients are final too (its own backward will find nothing to do)
        return (dx, dw, db_ret, None, None, None, dres) + (None,) * 12


# ---- fp32 inference path (csrc/f32_infer.hip): every op below accepts fp32 NHWC activations and then runs the fp32 kernels — forward
# only (the evaluation graphs; "eval box outputs within 1e-4 of the reference").  The TF variables are used as they are (no packing).
def _f32_infer(x):
    if x.dtype != torch.float32:
        return False
    if torch.is_grad_enabled() and x.requires_grad:
        raise RuntimeError("the fp32 path is inference only (run it under torch.no_grad())")
    return True


def _conv2d_f32(x, w, b, stride, relu, residual, padding):
    N, H, W, C = x.shape
    kh, kw, cin, cout = w.shape
    assert cin == C and x.is_contiguous(), "fp32 conv: input channels must match the kernel (no channel padding on this path)"
    d = _desc(N, H, W, C, cout, kh, kw, stride, padding == "valid")
    y = torch.empty((N, d.Ho, d.Wo, cout), dtype=torch.float32, device=x.device)
    call("danhip_conv2d_fwd_f32", ctypes.byref(d), ptr(x), ptr(w.detach().contiguous()), ptr(b.detach()) if b is not None else None, ptr(y), int(relu),
         ptr(residual.contiguous()) if residual is not None else None, stream())
    return y


# ---- split-operand inference (csrc/split_infer.hip): the fp32 path's convolutions at the 16-bit MFMA rate.  fp32 NHWC tensors stay the
# currency between ops (every non-convolution op is the fp32 path's); a convolution takes its input in the 3C half layout [hi | lo | hi]
# — from the producing convolution's epilogue when it left one behind (`_dh_split3`), else converted here — and runs the fp16 build's
# ordinary kernels over 3C input channels with weights [hi | hi | lo].
#
# Range.  Half limbs carry 22 significand bits only where both are normal numbers and hi is finite: |v| in [2^-3, 65504].  So every
# operand is moved there by a power of two (exact, and undone exactly in fp32):
#   - weights: per tensor, max|w * 2^e| in [2^13, 2^14) (_split_weight); the epilogue multiplies the accumulator by 2^-e;
#   - maps: a limb map holds x * 2^-LIMB_EXP (the exponent rides on the limb view as `_dh_exp`), so maps of magnitude up to
#     65504 * 2^LIMB_EXP = 262080 are carried; below 2^(LIMB_EXP-3) = 0.5 the lo limb is subnormal (absolute step 2^-22 of the value).
# A value outside that range (or a NaN) raises a device flag in whichever kernel writes the limbs; split_range_check() reads it and raises
# SplitRangeError (the models call it at the end of a "split" forward pass: net/sfd_net.py precision_scope).
LIMB_EXP = 2
_SPLIT_W = {}                # id(variable) -> (stamp, weakref, (packed fp16 weights, exponent)): evaluation weights are static, packed once
_RANGE_FLAG = [None]         # the int32 device flag registered with both libraries (danhip_split_set_range_flag)


class SplitRangeError(FloatingPointError):
    """A split-operand evaluation met a value outside the limbs' range (|x| >= 65520 * 2^exponent of its map, or NaN): its result is void."""


def _range_flag(device):
    f = _RANGE_FLAG[0]
    if f is None or f.device != device:
        f = torch.zeros(1, dtype=torch.int32, device=device)
        call("danhip_split_set_range_flag", ptr(f))
        _lib.call_f16("danhip_split_set_range_flag", ptr(f))
        _RANGE_FLAG[0] = f
    return f


def split_range_reset():
    """Clears the range flag (asynchronously, on the current stream) - at the start of an evaluation, so that a flag left behind by an aborted
    or unchecked call is not charged to it."""
    f = _RANGE_FLAG[0]
    if f is not None:
        f.zero_()


def split_range_check():
    """Raises SplitRangeError when a limb writer met a value outside the limbs' range since the last check (and clears the flag).  Waits for
    the current stream."""
    f = _RANGE_FLAG[0]
    if f is not None and int(f.item()):
        f.zero_()
        raise SplitRangeError("split-operand evaluation: a value outside the half limbs' range (|x| >= 65520 * 2^exponent of its map, or NaN); "
                              "the result would be silently wrong - evaluate with precision='fp32'")


def _weight_exp(w):
    """e with max|w * 2^e| in [2^13, 2^14) (0 for an all-zero tensor): frexp's exponent, so exactly e - s for w * 2^s."""
    import math
    m = float(w.detach().abs().max())
    if m == 0.0 or not math.isfinite(m):
        return 0
    return 14 - math.frexp(m)[1]


def _split_weight(d3, w, cin):
    """HWIO fp32 [kh, kw, cin, cout] -> (the fp16 build's forward packing of [w_hi | w_hi | w_lo | 0] of w * 2^e over d3.Cin = 3 cin
    (+ padding) channels, e)."""
    import weakref
    key = id(w)
    stamp = (WEIGHT_EPOCH, w._version, w.data_ptr(), d3.Cin)
    e = _SPLIT_W.get(key)
    if e is not None and e[0] == stamp and e[1]() is w:
        return e[2]
    ex = _weight_exp(w)
    wd = w.detach().float() * 2.0 ** ex                     # (exact)
    hi = wd.half().float()
    lo = (wd - hi).half().float()
    w3 = torch.cat([hi, hi, lo], dim=2).contiguous()
    r, c = ctypes.c_int64(), ctypes.c_int64()
    _lib.call_f16("danhip_conv_packed_dims", ctypes.byref(d3), 0, ctypes.byref(r), ctypes.byref(c))
    wf = torch.empty((r.value, c.value), dtype=torch.float16, device=w.device)
    _lib.call_f16("danhip_pack_conv_weight", ctypes.byref(d3), ptr(w3), 3 * cin, ptr(wf), None, stream())
    if isinstance(w, torch.nn.Parameter) or hasattr(w, "_danhip_grad") or getattr(w, "_dh_static", False):
        _SPLIT_W[key] = (stamp, weakref.ref(w, lambda _r, k=key: _SPLIT_W.pop(k, None)), (wf, ex))
    return wf, ex


_CAT_STATIC = {}


def cat_static(parts, dim):
    """torch.cat(parts, dim).contiguous(); during a split-operand evaluation without autograd the SAME tensor while no part changed, so that
    its limb packing and weight exponent are computed once (_split_weight: a fresh concatenation per call would cost a host round trip
    for its exponent)."""
    if not (_CTX.SPLIT_EVAL and not torch.is_grad_enabled()):
        return torch.cat(parts, dim).contiguous()
    key = (tuple(id(p) for p in parts), dim)
    stamp = (WEIGHT_EPOCH,) + tuple((p._version, p.data_ptr()) for p in parts)
    e = _CAT_STATIC.get(key)
    if e is not None and e[0] == stamp and all(r() is p for r, p in zip(e[2], parts)):
        return e[1]
    import weakref
    t = torch.cat(parts, dim).contiguous()
    t._dh_static = True
    evict = lambda _r, k=key: _CAT_STATIC.pop(k, None)         # the entry goes when any of its parts does
    _CAT_STATIC[key] = (stamp, t, tuple(weakref.ref(p, evict) for p in parts))
    return t


def _split_bias(b, exp):
    """b * 2^-exp in fp32 (exact), cached like the packed weights for parameters."""
    import weakref
    if exp == 0:
        return b.detach().float()
    key = ("bias", id(b))
    stamp = (WEIGHT_EPOCH, b._version, b.data_ptr(), exp)
    e = _SPLIT_W.get(key)
    if e is not None and e[0] == stamp and e[1]() is b:
        return e[2]
    bs = b.detach().float() * 2.0 ** -exp
    if isinstance(b, torch.nn.Parameter) or hasattr(b, "_danhip_grad") or getattr(b, "_dh_static", False):
        _SPLIT_W[key] = (stamp, weakref.ref(b, lambda _r, k=key: _SPLIT_W.pop(k, None)), bs)
    return bs


def _limb_view(x3, C, exp=0):
    """The tensor a split-mode convolution hands on: shape [.., C] (the nets read channel counts from it), IEEE half, a strided view of the
    HI limbs of the [.., 3C] limb-layout map, which rides along as `_dh_split3`, with its exponent `_dh_exp` (the limbs hold x * 2^-exp).
    Consumers inside this module: conv2d, max_pool_2x2 and l2_normalize take the limb layout as it is; every other op widens it to fp32
    first (_f32_in)."""
    v = x3[..., :C]
    v._dh_split3 = x3
    v._dh_exp = exp
    return v


def _is_limbs(x):
    return getattr(x, "_dh_split3", None) is not None


def _limb_exp(x):
    return getattr(x, "_dh_exp", 0)


def unsplit3(x):
    """limb view -> contiguous fp32 NHWC (hi + lo) * 2^exp."""
    x3 = x._dh_split3
    C = x.shape[-1]
    y = torch.empty(tuple(x.shape), dtype=torch.float32, device=x.device)
    call("danhip_unsplit3_scaled_f32", ptr(x3), ptr(y), y.numel() // C, C, x3.shape[-1], _limb_exp(x), stream())
    return y


def stop_gradient(x):
    """tf.stop_gradient.  A limb view (split-operand inference: nothing is differentiated) passes through — Tensor.detach() would return a
    plain half tensor without the limb map riding on it."""
    return x if _is_limbs(x) else x.detach()


def _f32_in(*ts):
    """Inputs of an op of the fp32 inference path: limb views (split-operand mode) widened to fp32, everything else untouched."""
    out = tuple(unsplit3(t) if (t is not None and _is_limbs(t)) else t for t in ts)
    return out[0] if len(out) == 1 else out


def split3(x, exp=0):
    """fp32 NHWC [.., C] -> IEEE-half [.., C3] = [hi | lo | hi | 0-padding] of x * 2^-exp, C3 = 3C rounded up to 8 (a limb view: its own
    map, whatever exp says)."""
    if _is_limbs(x):
        return x._dh_split3
    _range_flag(x.device)
    C = x.shape[-1]
    C3 = (3 * C + 7) // 8 * 8
    x3 = torch.empty(x.shape[:-1] + (C3,), dtype=torch.float16, device=x.device)
    call("danhip_split3_f32", ptr(x.contiguous()), ptr(x3), x.numel() // C, C, C3, 0, -exp, stream())
    return x3


def _conv2d_split(x, w, b, stride, relu, residual, padding, want_f32=False):
    """-> fp32 [N,Ho,Wo,cout] when the caller asks for it (heads), has a residual, or cout is ragged; else the next convolution's limb
    layout written by the kernel's epilogue (DANHIP_SPLIT3), returned as a limb view."""
    N, H, W, C = x.shape
    kh, kw, cin, cout = w.shape
    assert cin == C, "split conv: input channels must match the kernel"
    _range_flag(x.device)
    if (C == 3 and cout == 64 and kh == 3 and kw == 3 and stride == 1 and padding == "same" and residual is None and not want_f32
            and not _is_limbs(x) and x.dtype == torch.float32):
        # the first layer: 27 products per output - an exact fp32 FMA chain written straight in the limb layout (split_infer.hip)
        y3 = torch.empty((N, H, W, 3 * cout), dtype=torch.float16, device=x.device)
        call("danhip_conv3x3_c3_f32_split3", ptr(x.contiguous()), ptr(w.detach().float().contiguous()), ptr(b.detach().float()) if b is not None else None,
             ptr(y3), N, H, W, cout, int(relu), -LIMB_EXP, stream())
        return _limb_view(y3, cout, LIMB_EXP)
    # tensors of the 16-bit kernels are addressed with 32-bit element offsets: 3C input channels (the deformable GEMM's 27 x 256 at 160 x 160)
    # or 3 Cout output limbs can exceed 2^31 elements at batch 16 — such a call runs in batch slices
    C3 = (3 * C + 7) // 8 * 8
    ho, wo = (((H - kh) // stride + 1), ((W - kw) // stride + 1)) if padding == "valid" else (-(-H // stride), -(-W // stride))
    nmax = ((1 << 31) - 1) // max(H * W * C3, ho * wo * 3 * ((cout + 7) // 8 * 8))
    if N > nmax >= 1:
        residual = _f32_in(residual)
        parts = [_conv2d_split(x[i:i + nmax] if not _is_limbs(x) else _limb_view(x._dh_split3[i:i + nmax], C, _limb_exp(x)), w, b, stride, relu,
                               None if residual is None else residual[i:i + nmax], padding, want_f32=True) for i in range(0, N, nmax)]
        return torch.cat(parts, dim=0)
    xe = _limb_exp(x) if _is_limbs(x) else LIMB_EXP
    x3 = split3(x, xe)
    d3 = _desc(N, H, W, x3.shape[-1], cout, kh, kw, stride, padding == "valid")
    wf, we = _split_weight(d3, w, cin)
    limbs = not want_f32 and residual is None and cout % 8 == 0 and N * d3.Ho * d3.Wo * 3 * cout < (1 << 31)
    if limbs:
        y = torch.empty((N, d3.Ho, d3.Wo, 3 * cout), dtype=torch.float16, device=x.device)
    else:
        y = torch.empty((N, d3.Ho, d3.Wo, cout), dtype=torch.float32, device=x.device)
    n = _lib.lib_f16().danhip_conv2d_workspace_bytes(ctypes.byref(d3), 0) if -(-(N * d3.Ho * d3.Wo) // 128) * -(-cout // 128) <= 160 else 0
    ws = torch.empty(n, dtype=torch.uint8, device=x.device) if n else None
    ye = LIMB_EXP if limbs else 0                        # the output map's exponent, folded into the epilogue's power of two and the bias
    _lib.call_f16("danhip_conv2d_fwd_split", ctypes.byref(d3), ptr(x3), ptr(wf), ptr(_split_bias(b, ye)) if b is not None else None, ptr(y),
                  SPLIT3 if limbs else F32, int(relu), xe - we - ye, ptr(ws), n, stream())
    if limbs:
        return _limb_view(y, cout, LIMB_EXP)
    if residual is not None:                             # (added after the activation, as the 16-bit kernels' fused residual is)
        y.add_(_f32_in(residual))
    return y


def conv2d(x, w, b=None, stride=1, relu=False, out_f32=False, residual=None, pool=False, padding="same", pool_only=False, dy_slot=False):
    """dy_slot=True (with out_f32, a head convolution): the fp32 output carries a slot (`_dh_hslot`) through which heads_split hands this
    layer's channel-padded 16-bit dY over in backward, ready for the data and weight gradients.
    pool=True: also computes max_pool_2x2(y) (danhip_conv2d_fwd_pool); the next ops.max_pool_2x2(y) call picks it up.
    pool_only=True (with pool, no gradient tracked): the caller promises that ONLY the pooled map is used - where the kernel pools in its
    epilogue the full-resolution activation is never written and the POOLED tensor is returned (ops.max_pool_2x2 passes it through)."""
    if _is_limbs(x) or (_CTX.SPLIT_EVAL and _f32_infer(x)):
        return _conv2d_split(x, w, b, stride, relu, residual, padding, want_f32=out_f32)
    if _f32_infer(x):
        return _conv2d_f32(x, w, b, stride, relu, _f32_in(residual), padding)
    wp, bp = _param_handle(w), _param_handle(b)
    track = torch.is_grad_enabled() and (x.requires_grad or w.requires_grad or _sink_trainable(w))
    if track and relu and residual is not None:
        raise NotImplementedError("relu + fused residual needs a separate ReLU mask in backward (y > 0 is not the mask)")
    yslot = _new_slot(track and not out_f32)
    hslot = None
    if dy_slot and out_f32 and not relu and residual is None:
        yslot = hslot = _new_slot(track)
    pool_out = [] if (pool and relu and not out_f32 and residual is None and b is not None and w.shape[-1] % 8 == 0) else None
    if padding not in ("same", "valid"):
        raise ValueError("padding must be 'same' or 'valid'")
    blk = 0
    if torch.is_grad_enabled():
        blk = (1 if _sink_trainable(w) else 0) | (2 if (b is not None and _sink_trainable(b)) else 0)
    xs = _slot_of(x) if track else None
    xbits = _bits_holder(x) if (xs is not None and xs.is_relu and _CTX.USE_RELU_BITS) else None
    bits_out = [] if (track and relu and _CTX.USE_RELU_BITS) else None
    # pool_only: 1 = nothing tracked, the pooled map is returned; 2 = training with the direct gradient hand-off: y is declared but never written
    # (POOL_ONLY_TRAIN; off while a test records activations through TRACE)
    po = (1 if not track else (2 if (_CTX.POOL_ONLY_TRAIN and _CTX.TRACE is None and _CTX.USE_SLOTS and yslot is not None) else 0)) if pool_only else 0
    y = _Conv2d.apply(x, w, b, stride, relu, out_f32, residual, wp, bp, xs, yslot, pool_out, padding == "valid", blk, xbits, bits_out,
                      po, bool(track), getattr(x, "_dh_first", None) if track else None)
    if (track and relu and not x.requires_grad and wp is not None and x.shape[-1] == 8 and w.shape[2] <= 4 and w.shape[3] == 64 and w.shape[0] == 3
            and w.shape[1] == 3 and stride == 1 and padding == "same" and residual is None and not out_f32):
        y._dh_first = (x, wp, bp, w.shape[2])               # the first layer (image in, no data gradient): its consumer may fold its weight gradient in
    if getattr(y, "_dh_already_pooled", False):
        return y
    if _CTX.TRACE is not None and relu and wp is not None:
        _CTX.TRACE[id(wp)] = y.detach()
    if bits_out:                                         # the forward kernel wrote the masks: the holders of y (and its pooled map) start filled
        y._dh_bits = [bits_out[0]]
    if hslot is not None:
        _publish(y, hslot, False, _pad8(w.shape[-1]), ACT)
    else:
        _publish(y, yslot, relu, _ragged(w.shape[-1]))
    if pool_out:
        y._dh_pooled = pool_out[0]
        y._dh_pool_arg = pool_out[1]                     # 2-bit arg-max codes of the fused pool (None when nothing is tracked)
        if bits_out and bits_out[1] is not None:
            y._dh_pooled_bits = bits_out[1]
    return y


class _MaxPool(torch.autograd.Function):
    """tf.layers.max_pooling2d([2,2],[2,2],'same') — net/sfd_net.py:132."""

    @staticmethod
    def forward(ctx, x, xslot, yslot, pre=None, arg=None):
        N, H, W, C = x.shape
        if pre is not None:                              # already computed by the producing conv's epilogue (with its arg-max codes)
            y = pre
        else:
            y = torch.empty((N, (H + 1) // 2, (W + 1) // 2, C), dtype=x.dtype, device=x.device)
            arg = _pool_arg_buffer(y, x.requires_grad and C % 8 == 0)
            call("danhip_maxpool2x2_fwd_arg", ptr(x), ptr(y), ptr(arg), N, H, W, C, stream())
        ctx.arg = arg
        ctx.save_for_backward(x if arg is None else None)
        ctx.dims = (N, H, W, C)
        ctx.xslot, ctx.yslot = xslot, yslot
        if xslot is not None and arg is not None:
            xslot.taps |= TAP_POOL
        ctx.set_materialize_grads(False)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        N, H, W, C = ctx.dims
        g = _incoming(ctx.yslot, dy)
        if g is None:
            return None, None, None, None, None

        def scatter(dst, acc):
            if ctx.arg is not None:                      # through the forward pass's arg-max codes: the activation is not read again
                call("danhip_maxpool2x2_bwd_arg", ptr(ctx.arg), ptr(g), ptr(dst), N, H, W, C, acc, stream())
            else:
                call("danhip_maxpool2x2_bwd", ptr(x), ptr(g), ptr(dst), N, H, W, C, acc, stream())

        # the pooled maximum is > 0 exactly where its source is, so a gradient masked at the pooled level scatters to an already
        # ReLU-masked gradient; an unmasked one (autograd path) is masked by the producer's own backward, so it goes there by autograd
        xs = ctx.xslot if (ctx.xslot is not None and _pool_deliver_ok(ctx, dy)) else None
        if xs is not None:
            if ctx.arg is not None and _junction_ok(xs, dy, C):
                first = xs.pop_pending(TAP_L2NORM)
                if first is not None:                    # the L2-norm branch is waiting: both gradients in one pass, dx written once
                    buf, _ = xs.target()
                    _junction(first[1], (ctx.arg, g, (N, H, W, C)), buf, first[0], xs.is_relu, 0)
                elif xs.pending is None:                 # first of the two to arrive
                    xs.defer(TAP_POOL, scatter, (ctx.arg, g, (N, H, W, C)))
                else:
                    scatter(*xs.target())
                return None, None, None, None, None
        return _deliver(xs, (N, H, W, C), g, scatter), None, None, None, None


def _junction(l2, pool, buf, acc, is_relu, pool_first):
    """One launch for the two gradients of a tapped map (csrc/elementwise.hip, l2norm_bwd_pool_scatter_kernel)."""
    x, gamma, g, dg = l2
    arg, pg, (N, H, W, C) = pool
    if _CTX.deterministic:
        ws, nws = _reduce_ws(N * H * W, C, x.device)
        call("danhip_l2norm_bwd_pool_scatter_ws", ptr(x), ptr(gamma), ptr(g), ptr(arg), ptr(pg), ptr(buf), ptr(dg), N, H, W, C, acc,
             1 if is_relu else 0, pool_first, ptr(ws), nws, stream())
        return
    call("danhip_l2norm_bwd_pool_scatter", ptr(x), ptr(gamma), ptr(g), ptr(arg), ptr(pg), ptr(buf), ptr(dg), N, H, W, C, acc, 1 if is_relu else 0,
         pool_first, stream())


def _pool_deliver_ok(ctx, dy):
    # direct delivery into a ReLU slot requires every contribution to be masked already, i.e. no raw autograd gradient
    return not (ctx.xslot.is_relu and dy is not None)


def max_pool_2x2(x):
    if getattr(x, "_dh_already_pooled", False):           # conv2d(pool=True, pool_only=True) already returned the pooled map
        return x
    if _is_limbs(x):                                      # split-operand mode: pooled straight on the limb layout
        N, H, W, C = x.shape
        if C % 8 == 0 and x._dh_split3.shape[-1] == 3 * C:
            y3 = torch.empty((N, (H + 1) // 2, (W + 1) // 2, 3 * C), dtype=torch.float16, device=x.device)
            call("danhip_maxpool2x2_split3", ptr(x._dh_split3), ptr(y3), N, H, W, C, stream())
            return _limb_view(y3, C, _limb_exp(x))
        x = unsplit3(x)
    if _f32_infer(x):
        N, H, W, C = x.shape
        y = torch.empty((N, (H + 1) // 2, (W + 1) // 2, C), dtype=torch.float32, device=x.device)
        call("danhip_maxpool2x2_fwd_f32", ptr(x.contiguous()), ptr(y), N, H, W, C, stream())
        return y
    if _CTX.TRACE is not None:
        _CTX.TRACE.setdefault("pools", []).append(x.detach())
    track = torch.is_grad_enabled() and x.requires_grad
    xs = _slot_of(x) if track else None
    yslot = _new_slot(track)
    y = _MaxPool.apply(x, xs, yslot, getattr(x, "_dh_pooled", None), getattr(x, "_dh_pool_arg", None))
    pbits = getattr(x, "_dh_pooled_bits", None)
    if pbits is not None and getattr(x, "_dh_pooled", None) is not None:
        y._dh_bits = [pbits]                             # the fused conv + pool kernel also wrote the pooled map's ReLU bit mask
    return _publish(y, yslot, xs.is_relu if xs is not None else False)       # consumers may mask by (pooled > 0) when the source is a ReLU output


class _MaxPool3x3S2(torch.autograd.Function):
    """tf.layers.max_pooling2d([3,3],[2,2],'same') — net/resnet_danet.py:129."""

    @staticmethod
    def forward(ctx, x):
        N, H, W, C = x.shape
        y = torch.empty((N, (H + 1) // 2, (W + 1) // 2, C), dtype=x.dtype, device=x.device)
        call("danhip_maxpool3x3s2_same_fwd", ptr(x), ptr(y), N, H, W, C, stream())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        N, H, W, C = x.shape
        dx = torch.empty_like(x)
        call("danhip_maxpool3x3s2_same_bwd", ptr(x), ptr(dy.contiguous()), ptr(dx), N, H, W, C, stream())
        return dx


def max_pool_3x3_s2(x):
    return _MaxPool3x3S2.apply(_f32_in(x))


class _L2Norm(torch.autograd.Function):
    """VGG16Backbone.l2_normalize — net/sfd_net.py:68-79."""

    @staticmethod
    def forward(ctx, x, gamma, g_param, xslot, yslot):
        y = torch.empty_like(x)
        M = x.numel() // x.shape[-1]
        call("danhip_l2norm_fwd", ptr(x), ptr(gamma.detach()), ptr(y), M, x.shape[-1], stream())
        ctx.save_for_backward(x, gamma.detach())
        ctx.g_param = g_param
        ctx.xslot, ctx.yslot = xslot, yslot
        if xslot is not None and x.dim() == 4:
            xslot.taps |= TAP_L2NORM
        ctx.set_materialize_grads(False)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma = ctx.saved_tensors
        M = x.numel() // x.shape[-1]
        g = _incoming(ctx.yslot, dy)
        if g is None:
            return None, None, None, None, None
        dg, dg_ret = _grad_target(ctx.g_param, gamma.shape, gamma.device)
        xs = ctx.xslot

        def alone(buf, acc):
            if _CTX.deterministic:
                ws, nws = _reduce_ws(M, x.shape[-1], x.device)
                call("danhip_l2norm_bwd_ws", ptr(x), ptr(gamma), ptr(g), ptr(buf), ptr(dg), M, x.shape[-1], acc,
                     1 if (xs is not None and xs.is_relu) else 0, ptr(ws), nws, stream())
                return
            call("danhip_l2norm_bwd", ptr(x), ptr(gamma), ptr(g), ptr(buf), ptr(dg), M, x.shape[-1], acc, 1 if (xs is not None and xs.is_relu) else 0,
                 stream())

        if xs is not None and _junction_ok(xs, dy, x.shape[-1]):
            first = xs.pop_pending(TAP_POOL)
            if first is not None:                        # the pool's scatter is waiting: both gradients in one pass, dx written once
                buf, _ = xs.target()
                _junction((x, gamma, g, dg), first[1], buf, first[0], xs.is_relu, 1)
                return None, dg_ret, None, None, None
            if dg_ret is None and xs.pending is None:
                # first of the two to arrive.  (Only with a gradient sink: a dgamma handed back to autograd must be complete on return.)
                xs.defer(TAP_L2NORM, alone, (x, gamma, g, dg))
                return None, dg_ret, None, None, None
        return _deliver(xs, x.shape, x, alone), dg_ret, None, None, None


def l2_normalize(x, gamma):
    if _is_limbs(x) and x.shape[-1] % 8 == 0 and x._dh_split3.shape[-1] == 3 * x.shape[-1]:
        C = x.shape[-1]                                      # split-operand mode: normalised on the limb layout, for the head convolution that follows
        y3 = torch.empty_like(x._dh_split3)
        _range_flag(x.device)
        call("danhip_l2norm_split3", ptr(x._dh_split3), ptr(gamma.detach().float()), ptr(y3), y3.numel() // (3 * C), C, _limb_exp(x), 0, stream())
        return _limb_view(y3, C)            # (|y| <= |gamma|: exponent 0)
    x = _f32_in(x)
    if _f32_infer(x):
        y = torch.empty_like(x)
        call("danhip_l2norm_fwd_f32", ptr(x.contiguous()), ptr(gamma.detach()), ptr(y), x.numel() // x.shape[-1], x.shape[-1], stream())
        return y
    track = torch.is_grad_enabled() and (x.requires_grad or gamma.requires_grad)
    yslot = _new_slot(track)
    y = _L2Norm.apply(x, gamma, gamma if isinstance(gamma, torch.nn.Parameter) else None, _slot_of(x) if track else None, yslot)
    return _publish(y, yslot, False)


class _HeadSplit(torch.autograd.Function):
    """Max-out + reshape_pred for one pyramid level (depth 1): head conv output fp32 [B,H,W,4+nneg+npos] ->
    writes loc[B, off:off+HW, :], cls[B, off:off+HW, :] of the concatenated prediction buffers
    (net/sfd_net.py:175-216; train_sfd.py:293-304)."""

    @staticmethod
    def forward(ctx, h, loc, cls, nneg, npos, off):
        B, H, W, Ch = h.shape
        A = loc.shape[1]
        call("danhip_head_split_fwd", ptr(h), ptr(loc), ptr(cls), B, H * W, Ch, nneg, npos, A, off, stream())
        ctx.save_for_backward(h)
        ctx.cfg = (nneg, npos, off, A)
        ctx.mark_dirty(loc, cls)
        return loc, cls

    @staticmethod
    def backward(ctx, dloc, dcls):
        (h,) = ctx.saved_tensors
        nneg, npos, off, A = ctx.cfg
        B, H, W, Ch = h.shape
        dy = torch.empty((B, H, W, Ch), dtype=torch.float32, device=h.device)
        call("danhip_head_split_bwd", ptr(h), ptr(dloc.contiguous()), ptr(dcls.contiguous()), ptr(dy), B, H * W, Ch, nneg, npos, A, off, stream())
        return dy, dloc, dcls, None, None, None


def head_split(h, loc, cls, nneg, npos, off):
    return _HeadSplit.apply(h, loc, cls, nneg, npos, off)


class _HeadsSplit(torch.autograd.Function):
    """Max-out + reshape_pred for ALL pyramid levels in one launch each way (OpsContext.HEADS_BATCHED): the head maps h_i fp32
    [B,H_i,W_i,4+nneg_i+npos_i] -> loc [B,A,4], cls [B,A,2], level after level along A (what a chain of _HeadSplit nodes writes).
    Backward forms every level's gradient, rounds it to 16 bits and stores it channel-padded into the slot of the level's head
    convolution (conv2d(dy_slot=True)) - what head_split_bwd + the convolution's cast_pad produced per level through an fp32 dY - and
    hands autograd nothing: each convolution's backward finds its dY in its slot.  One node per forward call receives dloc / dcls once,
    so several forwards per step (train_step_towers) never share state."""

    @staticmethod
    def forward(ctx, cfg, slots, *hs):
        B = hs[0].shape[0]
        levels = (_lib.HeadLevel * len(hs))()
        off = 0
        for e, h, (nneg, npos) in zip(levels, hs, cfg):
            assert h.dtype == torch.float32 and h.is_contiguous() and h.dim() == 4 and h.shape[0] == B, "heads_split: fp32 NHWC head maps of one batch"
            e.h, e.dy = h.data_ptr(), None
            e.HW, e.Ch, e.nneg, e.npos, e.off, e.co_pad = h.shape[1] * h.shape[2], h.shape[3], nneg, npos, off, 0
            off += e.HW
        loc = torch.empty((B, off, 4), dtype=torch.float32, device=hs[0].device)         # (every element is written: the levels tile [0, A))
        cls = torch.empty((B, off, 2), dtype=torch.float32, device=hs[0].device)
        call("danhip_heads_split_fwd", levels, len(hs), ptr(loc), ptr(cls), B, off, stream())
        ctx.save_for_backward(*hs)
        ctx.levels, ctx.slots, ctx.dims = levels, slots, (B, off)
        return loc, cls

    @staticmethod
    def backward(ctx, dloc, dcls):
        hs = ctx.saved_tensors
        B, A = ctx.dims
        assert dloc.dtype == torch.float32 and dcls.dtype == torch.float32 and dloc.shape == (B, A, 4) and dcls.shape == (B, A, 2)
        dloc, dcls = dloc.contiguous(), dcls.contiguous()
        if dloc.data_ptr() % 16:                         # (a view at an odd element offset: the kernel loads float4 / float2)
            dloc = dloc.clone()
        if dcls.data_ptr() % 8:
            dcls = dcls.clone()
        levels = ctx.levels
        for e, h, slot in zip(levels, hs, ctx.slots):
            buf, acc = slot.target()
            if acc:
                raise RuntimeError("heads_split: a head convolution's dY slot was filled before the heads' backward ran")
            e.h, e.dy, e.co_pad = h.data_ptr(), buf.data_ptr(), buf.shape[-1]
        call("danhip_heads_grad_pad", levels, len(hs), ptr(dloc), ptr(dcls), B, A, stream())
        return (None, None) + (None,) * len(hs)


def heads_split(hs, cfg):
    """Head maps of all levels (conv2d(out_f32=True, dy_slot=True)) + their (nneg, npos) -> (loc [B,A,4], cls [B,A,2]).
    HEADS_BATCHED: one launch for all levels each way; else, and where the batched form does not apply (more levels than the kernels'
    table holds, or gradients tracked without the direct hand-off), the per-level launches into zero-filled buffers."""
    track = torch.is_grad_enabled() and any(h.requires_grad for h in hs)
    slots = [getattr(h, "_dh_hslot", None) for h in hs]
    if _CTX.HEADS_BATCHED and len(hs) <= _lib.HEADS_MAX_LEVELS and (not track or all(s is not None for s in slots)):
        return _HeadsSplit.apply([tuple(c) for c in cfg], slots, *hs)
    B, dev = hs[0].shape[0], hs[0].device
    A = sum(h.shape[1] * h.shape[2] for h in hs)
    loc = torch.zeros((B, A, 4), dtype=torch.float32, device=dev)
    cls = torch.zeros((B, A, 2), dtype=torch.float32, device=dev)
    off = 0
    for h, (nneg, npos) in zip(hs, cfg):
        loc, cls = head_split(h, loc, cls, nneg, npos, off)
        off += h.shape[1] * h.shape[2]
    return loc, cls


class _DetectionLoss(torch.autograd.Function):
    """Hard-negative mining + CE*(ratio+1) + smooth-L1 (train_sfd.py:350-417 / train_dan.py:286-324,470-478).
    Returns a 4-vector acc = [ce_sum, n_selected, loc_sum, n_pos] (device, no sync); the loss is
    (ratio+1)*ce_sum/n_selected + loc_sum/n_pos.  backward() expects the upstream gradient of that 4-vector to be
    ignored: it uses ctx.scale (= d total_loss / d this loss term) instead."""

    @staticmethod
    def forward(ctx, cls, loc, labels, loc_t, ratio, at_least_one, scale, metric_counts=None):
        B, A, _ = cls.shape
        # the kernels read raw pointers: a wrong dtype would be misread silently
        assert cls.dtype == torch.float32 and loc.dtype == torch.float32 and loc_t.dtype == torch.float32, "detection_loss: fp32 logits / targets"
        assert labels.dtype == torch.int32 and labels.shape == (B, A), "detection_loss: labels must be int32 [B, A]"
        assert cls.is_contiguous() and loc.is_contiguous() and labels.is_contiguous() and loc_t.is_contiguous()
        dev = cls.device
        score = torch.empty((B, A), dtype=torch.float32, device=dev)
        counts = torch.empty((B, 2), dtype=torch.int32, device=dev)
        thr = torch.empty((B,), dtype=torch.float32, device=dev)
        k = torch.empty((B,), dtype=torch.int32, device=dev)
        sel = torch.empty((B, A), dtype=torch.uint8, device=dev)
        acc = torch.empty((4,), dtype=torch.float32, device=dev)
        call("danhip_hard_neg_select", ptr(cls), ptr(labels), ptr(score), ptr(counts), ptr(thr), ptr(k), B, A, float(ratio), int(at_least_one), stream())
        if _CTX.deterministic:
            nlws = int(_lib.lib().danhip_loss_workspace_bytes())
            lws = torch.empty((nlws,), dtype=torch.uint8, device=dev)
            call("danhip_detection_loss_fwd_ws", ptr(cls), ptr(loc), ptr(labels), ptr(loc_t), ptr(score), ptr(thr), ptr(sel), ptr(acc), B, A,
                 ptr(lws), nlws, stream())
        else:
            call("danhip_detection_loss_fwd", ptr(cls), ptr(loc), ptr(labels), ptr(loc_t), ptr(score), ptr(thr), ptr(sel), ptr(acc), B, A, stream())
        if _CTX.TRACE is not None:                           # tests: the hard-negative selection of this term (call order), imposed on the oracle's loss
            _CTX.TRACE.setdefault("loss_sel", []).append(sel)
        if metric_counts is not None:                        # the reference's cls_accuracy over this term's final_mask (one more launch; opt-in)
            cls_accuracy(cls, labels, sel, metric_counts)
        ctx.save_for_backward(cls, loc, loc_t, sel, acc)
        ctx.cfg = (ratio, scale)
        ctx.aux = (score, thr, k, counts)
        return acc

    @staticmethod
    def backward(ctx, dacc):
        cls, loc, loc_t, sel, acc = ctx.saved_tensors
        ratio, scale = ctx.cfg
        B, A, _ = cls.shape
        dcls = torch.empty_like(cls)
        dloc = torch.empty_like(loc)
        call("danhip_detection_loss_bwd", ptr(cls), ptr(loc), ptr(loc_t), ptr(sel), ptr(acc), ptr(dcls), ptr(dloc), float((ratio + 1.0) * scale),
             float(scale), B, A, stream())
        if _CTX.LOSS_SCALE_DEV is not None:                  # dynamic loss scale (fp16 build): a device scalar, so the step stays capturable
            dcls.mul_(_CTX.LOSS_SCALE_DEV)
            dloc.mul_(_CTX.LOSS_SCALE_DEV)
        return dcls, dloc, None, None, None, None, None, None


def detection_loss(cls, loc, labels, loc_t, ratio=3.0, at_least_one=False, scale=1.0, metric_counts=None):
    """metric_counts: None, or an int64 [2] device tensor {correct, total} that cls_accuracy adds this term's mined anchors to."""
    return _DetectionLoss.apply(cls, loc, labels, loc_t, ratio, at_least_one, scale, metric_counts)


def cls_accuracy(cls, labels, sel, counts):
    """The reference's streaming tf.metrics.accuracy (train_sfd.py:383-395) on the device: over the anchors with sel != 0 (final_mask, as
    detection_loss's forward wrote it), counts[0] += #(argmax(cls, -1) == clip(labels, 0, 2)) and counts[1] += their number.  cls fp32
    [B,A,2], labels int32 [B,A], sel uint8 [B,A], counts int64 [2] (added to: a running total the caller zeroes once).  One launch, no sync;
    integer sums, so the same bits with and without OpsContext.deterministic."""
    B, A, _ = cls.shape
    assert cls.dtype == torch.float32 and cls.shape[2] == 2 and labels.dtype == torch.int32 and labels.shape == (B, A), "cls_accuracy: fp32 [B,A,2] logits, int32 [B,A] labels"
    assert sel.dtype == torch.uint8 and sel.shape == (B, A) and counts.dtype == torch.int64 and counts.numel() == 2, "cls_accuracy: uint8 [B,A] sel, int64 [2] counts"
    assert cls.device == labels.device == sel.device == counts.device
    call("danhip_cls_accuracy", ptr(cls), ptr(labels), ptr(sel), ptr(counts), B, A, stream())
    return counts


def preprocess_u8(img_rgb_u8):
    """uint8 RGB [N,H,W,3] -> bf16 [N,H,W,8] (BGR - mean, zero padded): dan_preprocessing.py:55-57,755-758."""
    assert img_rgb_u8.dtype == torch.uint8 and img_rgb_u8.shape[-1] == 3
    N, H, W, _ = img_rgb_u8.shape
    out = torch.empty((N, H, W, 8), dtype=ACT, device=img_rgb_u8.device)
    call("danhip_preprocess_u8", ptr(img_rgb_u8.contiguous()), ptr(out), N * H * W, stream())
    return out


def cast_pad(x_f32, c_dst):
    """fp32 [..., C] -> bf16 [..., c_dst] zero padded."""
    shp = x_f32.shape
    rows = x_f32.numel() // shp[-1]
    out = torch.empty(shp[:-1] + (c_dst,), dtype=ACT, device=x_f32.device)
    call("danhip_cast_pad_f32_to_bf16", ptr(x_f32.contiguous()), None, ptr(out), rows, shp[-1], c_dst, stream())
    return out


class _ResizeAdd(torch.autograd.Function):
    """out = lateral + tf.image.resize_bilinear(up, size(lateral)) (TF1 legacy mapping) — the LFPN merge of
    net/pb_net.py:209-217 / net/danet.py:363-371.  lateral may be None (plain resize to `size`)."""

    @staticmethod
    def forward(ctx, up, lateral, size, yslot=None):
        N, Hi, Wi, C = up.shape
        ctx.yslot = yslot
        ctx.set_materialize_grads(False)
        Ho, Wo = (lateral.shape[1], lateral.shape[2]) if lateral is not None else size
        assert up.dtype == ACT and up.is_contiguous() and C % 8 == 0
        out = torch.empty((N, Ho, Wo, C), dtype=ACT, device=up.device)
        call("danhip_resize_bilinear_add_fwd", ptr(up), ptr(lateral.contiguous()) if lateral is not None else None, ptr(out), N, Hi, Wi, Ho, Wo, C, stream())
        ctx.dims = (N, Hi, Wi, Ho, Wo, C)
        ctx.has_lat = lateral is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        N, Hi, Wi, Ho, Wo, C = ctx.dims
        # the merged map feeds two convolutions in the LFPN (this level's fused 3x3 and the next level's upsample 1x1): both deliver into its
        # slot (write, then accumulate in the kernel epilogue) instead of returning two tensors for the autograd engine to add
        g = _incoming(ctx.yslot, dout)
        if g is None:
            return None, None, None, None
        dup = None
        if ctx.needs_input_grad[0]:
            dup = torch.empty((N, Hi, Wi, C), dtype=ACT, device=g.device)
            call("danhip_resize_bilinear_add_bwd", ptr(g), ptr(dup), N, Hi, Wi, Ho, Wo, C, 0, stream())
        return dup, (g if ctx.has_lat else None), None, None


def resize_bilinear_add(up, lateral=None, size=None):
    up, lateral = _f32_in(up, lateral)
    if _f32_infer(up):
        N, Hi, Wi, C = up.shape
        Ho, Wo = (lateral.shape[1], lateral.shape[2]) if lateral is not None else size
        out = torch.empty((N, Ho, Wo, C), dtype=torch.float32, device=up.device)
        call("danhip_resize_bilinear_add_fwd_f32", ptr(up.contiguous()), ptr(lateral.contiguous()) if lateral is not None else None, ptr(out), N, Hi, Wi,
             Ho, Wo, C, stream())
        return out
    track = torch.is_grad_enabled() and (up.requires_grad or (lateral is not None and lateral.requires_grad))
    yslot = _new_slot(track)
    return _publish(_ResizeAdd.apply(up, lateral, size, yslot), yslot, False)


# ---- transposed convolution 4 x 4 / stride 2 with the lateral add (csrc/conv_transpose.hip): the LFPN's learnable upsampling
_CT_PACKED = {}              # id(variable) -> [weakref, stamp, wf, wb]: the two 16-bit operands, keyed on the weight epoch like _PACKED


def _ct_pack(wd, need_bwd):
    if not (wd.dtype == torch.float32 and wd.is_contiguous()):
        raise RuntimeError("conv_transpose_add: the kernel variable must be a contiguous fp32 [4, 4, Cout, Cin] tensor")
    cout, cin = wd.shape[2], wd.shape[3]
    wf = torch.empty((4, 4, cout, cin), dtype=ACT, device=wd.device)
    wb = torch.empty((4, 4, cin, cout), dtype=ACT, device=wd.device) if need_bwd else None
    call("danhip_conv_transpose4x4s2_pack_weight", ptr(wd), ptr(wf), ptr(wb), cin, cout, stream())
    return wf, wb


def _ct_packed(w, w_param, need_bwd):
    """-> (wf [4,4,Cout,Cin], wb [4,4,Cin,Cout] or None), 16-bit: cached per variable while it is unchanged (_stamp), packed on the spot
    for a plain tensor."""
    if w_param is None:
        return _ct_pack(w.detach(), need_bwd)
    import weakref
    pid = id(w_param)
    e = _CT_PACKED.get(pid)
    st = _stamp(w_param) + (tuple(w_param.shape),)
    if e is None or e[0]() is not w_param or e[1] != st or (need_bwd and e[3] is None):
        wf, wb = _ct_pack(w_param.detach(), need_bwd or (e is not None and e[0]() is w_param and e[3] is not None))
        e = _CT_PACKED[pid] = [weakref.ref(w_param, lambda _r, pid=pid: _CT_PACKED.pop(pid, None)), st, wf, wb]
    return e[2], (e[3] if need_bwd else None)


def _ct_wgrad_scratch(dims, dev):
    key = ("ct",) + tuple(dims)
    n = _SCRATCH_BYTES.get(key)
    if n is None:
        n = _SCRATCH_BYTES[key] = int(_lib.lib().danhip_conv_transpose4x4s2_wgrad_workspace_bytes(*dims))
    return torch.empty(n, dtype=torch.uint8, device=dev), n


class _ConvTransposeAdd(torch.autograd.Function):
    """out = lateral + tf.layers.conv2d_transpose(up, Cout, (4, 4), strides=(2, 2), padding='same'), cropped top-left to the lateral's size
    (include/danhip.h has the rule).  One node: forward, data gradient (into the producer's slot) and weight / bias gradient (into the
    trainer's sinks, on the weight-gradient stream)."""

    @staticmethod
    def forward(ctx, up, w, b, lateral, size, w_param, b_param, xslot, yslot):
        N, Hi, Wi, Cin = up.shape
        Cout = w.shape[2]
        Ho, Wo = (lateral.shape[1], lateral.shape[2]) if lateral is not None else size
        assert up.dtype == ACT and up.is_contiguous(), "conv_transpose_add input must be contiguous NHWC 16-bit"
        need_bwd = up.requires_grad or w.requires_grad
        wf, wb = _ct_packed(w, w_param, need_bwd)
        out = torch.empty((N, Ho, Wo, Cout), dtype=ACT, device=up.device)
        call("danhip_conv_transpose4x4s2_add_fwd", ptr(up), ptr(wf), ptr(b.detach()) if b is not None else None,
             ptr(lateral.contiguous()) if lateral is not None else None, ptr(out), N, Hi, Wi, Ho, Wo, Cin, Cout, stream())
        ctx.dims = (N, Hi, Wi, Ho, Wo, Cin, Cout)
        ctx.xslot, ctx.yslot = xslot, yslot
        ctx.w_param, ctx.b_param = w_param, b_param
        ctx.has_lat, ctx.has_bias = lateral is not None, b is not None
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(up, wb)
        return out

    @staticmethod
    def backward(ctx, dout):
        up, wb = ctx.saved_tensors
        dims = ctx.dims
        N, Hi, Wi, Ho, Wo, Cin, Cout = dims
        # the merged map feeds two convolutions in the LFPN (this level's fused 3x3 and the next level's upsample 1x1): both deliver into its slot
        g = _incoming(ctx.yslot, dout)
        if g is None:
            return (None,) * 9
        dup = None
        if ctx.needs_input_grad[0]:
            def data_grad(buf, acc):
                call("danhip_conv_transpose4x4s2_dgrad", ptr(g), ptr(wb), ptr(buf), N, Hi, Wi, Ho, Wo, Cin, Cout, acc, stream())

            dup = _deliver(ctx.xslot, up.shape, up, data_grad)
        wp, bp = ctx.w_param, ctx.b_param
        need_dw = ctx.needs_input_grad[1]
        need_db = ctx.has_bias and ctx.needs_input_grad[2]
        dw = db_ret = None
        if need_dw or need_db:
            dw_to, dw = _grad_target(wp, (4, 4, Cout, Cin), g.device) if need_dw else (None, None)
            db_to, db_ret = _grad_target(bp, (Cout,), g.device) if need_db else (None, None)
            ws, nws = _ct_wgrad_scratch(dims, g.device)

            def issue(st):
                call("danhip_conv_transpose4x4s2_wgrad", ptr(up), ptr(g), ptr(dw_to), ptr(db_to), N, Hi, Wi, Ho, Wo, Cin, Cout, ptr(ws), nws, st)

            # (the side stream only when both gradients go to sinks: one handed back to autograd is consumed on this stream)
            _launch_wgrad(None, dw is None and db_ret is None, issue, (g, up, ws))
            if _CTX.GRAD_READY_HOOK is not None and wp is not None:
                _CTX.GRAD_READY_HOOK(wp)
        return dup, dw, db_ret, (g if ctx.has_lat else None), None, None, None, None, None


def conv_transpose_add(up, w, b, lateral=None, size=None):
    """lateral + conv2d_transpose(up; w [4, 4, Cout, Cin], b [Cout]; 4 x 4, stride 2, 'same'), at the lateral's size or `size` = (Ho, Wo):
    2 Hi x 2 Wi or one less each way (top-left crop).  The learnable counterpart of resize_bilinear_add."""
    if _is_limbs(up) or (lateral is not None and _is_limbs(lateral)) or (_CTX.SPLIT_EVAL and up.dtype == torch.float32):
        raise ValueError("conv_transpose_add (lfpn_upsample='transposed') has no split-operand form: precision='split' is not supported with it")
    N, Hi, Wi, Cin = up.shape
    if tuple(w.shape[:2]) != (4, 4) or w.shape[3] != Cin:
        raise ValueError("conv_transpose_add: the kernel must be [4, 4, Cout, %d], got %s" % (Cin, tuple(w.shape)))
    if lateral is None and size is None:
        size = (2 * Hi, 2 * Wi)
    if _f32_infer(up):
        Ho, Wo = (lateral.shape[1], lateral.shape[2]) if lateral is not None else size
        out = torch.empty((N, Ho, Wo, w.shape[2]), dtype=torch.float32, device=up.device)
        call("danhip_conv_transpose4x4s2_add_fwd_f32", ptr(up.contiguous()), ptr(w.detach().contiguous()), ptr(b.detach()) if b is not None else None,
             ptr(lateral.contiguous()) if lateral is not None else None, ptr(out), N, Hi, Wi, Ho, Wo, Cin, w.shape[2], stream())
        return out
    track = torch.is_grad_enabled() and (up.requires_grad or w.requires_grad or (lateral is not None and lateral.requires_grad))
    yslot = _new_slot(track)
    xs = _slot_of(up) if track else None
    if xs is not None and xs.is_relu:
        xs = None                # (no ReLU mask in this data gradient's epilogue: the gradient of a ReLU output travels through autograd)
    return _publish(_ConvTransposeAdd.apply(up, w, b, lateral, size, _param_handle(w), _param_handle(b), xs, yslot), yslot, False)


class _AvgPool2x2S1(torch.autograd.Function):
    """tf.layers.average_pooling2d((2,2), 1, 'same') — net/danet.py:854."""

    @staticmethod
    def forward(ctx, x, xslot, yslot):
        N, H, W, C = x.shape
        y = torch.empty_like(x)
        call("danhip_avgpool2x2s1_same_fwd", ptr(x), ptr(y), N, H, W, C, stream())
        ctx.dims = (N, H, W, C)
        ctx.xslot, ctx.yslot = xslot, yslot
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x if (xslot is not None and xslot.is_relu) else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, H, W, C = ctx.dims
        g = _incoming(ctx.yslot, dy)
        if g is None:
            return None, None, None
        (x,) = ctx.saved_tensors                         # (kept only where the producer's slot wants its ReLU backward folded in)

        def launch(buf, acc):
            call("danhip_avgpool2x2s1_same_bwd", ptr(g), ptr(x), ptr(buf), N, H, W, C, acc, stream())

        return _deliver(ctx.xslot, (N, H, W, C), g, launch), None, None


def avg_pool_2x2_s1(x):
    x = _f32_in(x)
    if _f32_infer(x):
        N, H, W, C = x.shape
        y = torch.empty_like(x)
        call("danhip_avgpool2x2s1_same_fwd_f32", ptr(x.contiguous()), ptr(y), N, H, W, C, stream())
        return y
    assert x.dtype == ACT and x.is_contiguous() and x.shape[-1] % 8 == 0
    track = torch.is_grad_enabled() and x.requires_grad
    yslot = _new_slot(track)
    return _publish(_AvgPool2x2S1.apply(x, _slot_of(x) if track else None, yslot), yslot, False)


class _Concat(torch.autograd.Function):
    """tf.concat(values, axis=-1) (net/danet.py:911, :951; net/pb_net.py:306).  Backward hands each input its slice of dY directly
    (one pass: slice + the input's ReLU backward + accumulate), instead of autograd's strided views + .contiguous() + clone + mask."""

    @staticmethod
    def forward(ctx, slots, yslot, all_relu, *xs):
        y = torch.cat(xs, dim=-1)
        ctx.slots, ctx.yslot, ctx.all_relu = slots, yslot, all_relu
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(*[x if (s is not None and s.is_relu) else None for x, s in zip(xs, slots)])
        ctx.widths = [x.shape[-1] for x in xs]
        return y

    @staticmethod
    def backward(ctx, dy):
        premasked = ctx.all_relu and dy is None          # slot deliveries arrive multiplied by (y > 0) = every input's own mask
        g = _incoming(ctx.yslot, dy, torch.Tensor.contiguous, ragged=True)       # (ragged output width: the slot carries the channel-padded layout)
        if g is None:
            return (None,) * (3 + len(ctx.widths))
        grads, c0 = [], 0
        for i, (C, s, x) in enumerate(zip(ctx.widths, ctx.slots, ctx.saved_tensors)):
            if not ctx.needs_input_grad[3 + i]:
                grads.append(None)
            elif s is None:
                grads.append(g[..., c0:c0 + C])
            else:
                buf, acc = s.target()
                call("danhip_slice_deliver", ptr(g), g.shape[-1], c0, C, ptr(x) if (s.is_relu and not premasked) else None, C, ptr(buf),
                     buf.shape[-1], acc, g.numel() // g.shape[-1], stream())
                grads.append(None)
            c0 += C
        return (None, None, None) + tuple(grads)


def concat(tensors):
    """Channel concatenation of NHWC activations."""
    tensors = [_f32_in(t) for t in tensors]
    track = torch.is_grad_enabled() and any(t.requires_grad for t in tensors)
    if tensors[0].dtype != ACT or not track or not _CTX.USE_SLOTS:
        return torch.cat(tensors, dim=-1)
    slots = [(getattr(t, "_dh_slot", None) or getattr(t, "_dh_pslot", None)) if t.requires_grad else None for t in tensors]
    all_relu = all(s is not None and s.is_relu for s in slots)
    yslot = _new_slot(True)
    y = _Concat.apply(slots, yslot, all_relu, *tensors)
    return _publish(y, yslot, all_relu, _ragged(y.shape[-1]))       # ragged width: consumers deliver into the channel-padded layout


class _Add(torch.autograd.Function):
    """a + b of two activations (the context module's residual, net/danet.py:913-918 / net/danet_deform.py:286-290): one library kernel forward
    (danhip_add16); backward delivers dY into both producers' slots, each with its own ReLU backward folded in — in ONE pass over dY
    (danhip_residual_bwd) when `a` is a ReLU output receiving its first delivery (the shape of every residual in the reference graphs)."""

    @staticmethod
    def forward(ctx, a, b, sa, sb, yslot):
        ctx.slots, ctx.yslot = (sa, sb), yslot
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(*[t if (s is not None and s.is_relu) else None for t, s in ((a, sa), (b, sb))])
        if a.dtype == ACT and a.is_contiguous() and b.is_contiguous() and a.is_cuda and a.numel() % 8 == 0:
            out = torch.empty_like(a)
            call("danhip_add16", ptr(a), ptr(b), ptr(out), a.numel(), stream())
            return out
        return a + b

    @staticmethod
    def backward(ctx, dy):
        g = _incoming(ctx.yslot, dy)
        if g is None:
            return (None,) * 5
        sa, sb = ctx.slots
        ta, tb = ctx.saved_tensors
        if (sa is not None and sb is not None and sa.is_relu and ctx.needs_input_grad[0] and ctx.needs_input_grad[1] and sa.buf is None
                and g.numel() % 8 == 0):
            bufa, _ = sa.target()                                # first delivery into a's slot: written, not accumulated
            bufb, accb = sb.target()
            call("danhip_residual_bwd", ptr(g), ptr(ta), ptr(tb) if sb.is_relu else None, ptr(bufa), ptr(bufb), accb, g.numel(), stream())
            return None, None, None, None, None
        out = []
        for i, (s, t) in enumerate(zip(ctx.slots, ctx.saved_tensors)):
            if not ctx.needs_input_grad[i]:
                out.append(None)
            elif s is None:
                out.append(g)
            else:
                buf, acc = s.target()
                C = g.shape[-1]
                call("danhip_slice_deliver", ptr(g), C, 0, C, ptr(t) if s.is_relu else None, C, ptr(buf), C, acc, g.numel() // C, stream())
                out.append(None)
        return out[0], out[1], None, None, None


def add(a, b):
    a, b = _f32_in(a, b)
    track = torch.is_grad_enabled() and (a.requires_grad or b.requires_grad)
    if a.dtype != ACT or not track or not _CTX.USE_SLOTS or a.shape != b.shape or a.shape[-1] % 8:
        return a + b
    yslot = _new_slot(True)
    return _publish(_Add.apply(a, b, _slot_of(a) if a.requires_grad else None, _slot_of(b) if b.requires_grad else None, yslot), yslot, False)


def _vptr(t):
    """Device pointer of an NHWC activation that may be a CHANNEL-SLICE VIEW of a wider tensor (dense channel axis, pixels t.stride(-2)
    elements apart): what the *_strided entry points take together with that pitch."""
    assert t.dim() == 4 and t.stride(3) == 1, "channel-slice view: NHWC with a dense channel axis"
    N, H, W, _ = t.shape
    ld = t.stride(2)
    assert ld % 8 == 0 and t.stride(1) == W * ld and t.stride(0) == H * W * ld and t.storage_offset() % 8 == 0, "not a channel slice of a contiguous NHWC tensor"
    return ctypes.c_void_p(t.data_ptr())


def _wgrad_launch(d, xv, dyv, dw, db, cin_real, keep):
    """Weight (+ bias) gradient of descriptor d with x / dy given as (possibly channel-slice) views, on the weight-gradient stream
    whenever the trainer has it on (these callers' gradients back to autograd, if any, are complete at the join like the sinks)."""
    pitch = _lib.ConvPitch(xv.stride(2), dyv.stride(2), 0)
    ws, nws = _wgrad_scratch(d, dyv.device)

    def issue(st):
        call("danhip_conv2d_bwd_weight_strided", ctypes.byref(d), _vptr(xv), _vptr(dyv), ptr(dw), ptr(db), cin_real, ctypes.byref(pitch), ptr(ws), nws, st)

    _launch_wgrad(d, True, issue, (xv, dyv, ws) + tuple(keep))


class _ContextBlock(torch.autograd.Function):
    """DAN context module V1, se_inception_block (net/danet.py:842-918), as ONE autograd node over channel-slice views — round 4.

    Forward (8 launches instead of 13 + torch.cat + torch add):
        hyper[.., 0:64]      = relu(conv1x1_b1(x))                                   written straight into the concat buffer
        T = [b3 | b4 | p2]   = conv1x1(x) with the three kernels side by side (192 columns; ReLU on the first 128 only)
        hyper[.., 64:128]    = relu(avg_pool_2x2_s1(p2))        branch 2's 1x1 commuted in front of the (linear) pool: conv(avg(x)) = avg(conv(x)),
                                                                its bias included (the average of a constant is the constant)
        hyper[.., 128:192]   = relu(conv3x1(b3)) | relu(conv1x3(b3))                 ONE 3x3 convolution 64 -> 64 whose kernel holds the 3x1 taps in its
                                                                middle column for outputs 0..31 and the 1x3 taps in its middle row for outputs 32..63,
                                                                zeros elsewhere ("plus" block of the flat buffers): the register-resident 64 -> 64 kernel
                                                                (conv_halo_c64.hip) and the row-streaming weight gradient take it on the large levels
        U                    = relu(conv3x3(b4));  hyper[.., 192:256] = relu(conv3x1(U)) | relu(conv1x3(U))       (the same way)
        out                  = relu(conv1x1_res(hyper)) + x
    Backward: d hyper comes out of the residual conv's data gradient already multiplied by (hyper > 0) = every branch's own ReLU mask;
    each branch convolution reads ITS slice of it in place (no slice copies), gradients meet in dT / dU by accumulation, and x receives
    three deliveries (skip path, fused 1x1, b1) instead of seven.  Variable names, creation order and arithmetic per output element are
    the reference's."""

    @staticmethod
    def forward(ctx, x, xslot, yslot, handles, hook_order, *wb):
        N, H, W, C = x.shape
        dev = x.device
        assert x.dtype == ACT and x.is_contiguous() and C % 64 == 0
        pairs = list(zip(wb[0::2], wb[1::2]))                       # b1, cat, b3 plus (3x1 | 1x3), b43, b4 plus, res
        need_bwd = any(t.requires_grad for t in wb) or x.requires_grad or any(_sink_trainable(t) for t in wb)
        T = torch.empty((N, H, W, 192), dtype=ACT, device=dev)
        hyper = torch.empty((N, H, W, 256), dtype=ACT, device=dev)
        U = torch.empty((N, H, W, 64), dtype=ACT, device=dev)
        r = torch.empty((N, H, W, C), dtype=ACT, device=dev)
        out = torch.empty((N, H, W, C), dtype=ACT, device=dev)
        descs, wbs = [], []

        def conv(i, xv, yv, kh, kw, relu_ch):
            w, b = pairs[i]
            d = _desc(N, H, W, xv.shape[-1], yv.shape[-1], kh, kw, 1)
            wf, wbk = packed_weights(d, w, handles[i][0], need_bwd)
            pitch = _lib.ConvPitch(xv.stride(2), yv.stride(2), 0)
            sc, nsc = _conv_scratch(d, 0, dev)
            e0 = _prof_begin()
            call("danhip_conv2d_fwd_strided", ctypes.byref(d), _vptr(xv), ptr(wf), ptr(b.detach()), _vptr(yv), 1, relu_ch, ctypes.byref(pitch), ptr(sc), nsc,
                 stream())
            _prof_end(e0, d, 0)
            descs.append(d)
            wbs.append(wbk)

        conv(0, x, hyper[..., 0:64], 1, 1, 64)
        conv(1, x, T, 1, 1, 128)
        call("danhip_avgpool2x2s1_same_fwd_strided", _vptr(T[..., 128:192]), 192, _vptr(hyper[..., 64:128]), 256, N, H, W, 64, 1, stream())
        conv(2, T[..., 0:64], hyper[..., 128:192], 3, 3, 64)
        conv(3, T[..., 64:128], U, 3, 3, 64)
        conv(4, U, hyper[..., 192:256], 3, 3, 64)
        conv(5, hyper, r, 1, 1, C)
        call("danhip_add16", ptr(r), ptr(x), ptr(out), out.numel(), stream())
        ctx.descs, ctx.handles, ctx.hook_order = descs, handles, hook_order
        ctx.xslot, ctx.yslot = xslot, yslot
        ctx.nw = len(wb)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, T, hyper, U, r, *wbs)
        ctx.blocks = [(_sink_trainable(w), _sink_trainable(b)) for w, b in pairs]
        ctx.cin_real = [w.shape[2] for w, _ in pairs]
        ctx.couts = [w.shape[3] for w, _ in pairs]
        ctx.khw = [(w.shape[0], w.shape[1]) for w, _ in pairs]
        if _CTX.TRACE is not None:                           # the block's ten ReLU decisions (tests): context_block() files them under their kernel variables
            _CB_LAST.clear()
            _CB_LAST.update({"b1": hyper[..., 0:64], "b2": hyper[..., 64:128], "b3": T[..., 0:64], "b3a": hyper[..., 128:160], "b3b": hyper[..., 160:192],
                             "b4": T[..., 64:128], "b43": U, "b4a": hyper[..., 192:224], "b4b": hyper[..., 224:256], "res": r})
        return out

    @staticmethod
    def backward(ctx, dy):
        x, T, hyper, U, r = ctx.saved_tensors[:5]
        wbs = ctx.saved_tensors[5:]
        N, H, W, C = x.shape
        dev = x.device
        g = _incoming(ctx.yslot, dy)
        if g is None:
            return (None,) * (5 + ctx.nw)
        xs = ctx.xslot
        need_dx = ctx.needs_input_grad[0]
        xmask = x if (need_dx and xs is not None and xs.is_relu) else None
        xbuf = None
        gr = torch.empty_like(g)

        def skip_path(buf, acc):                         # the first of x's three deliveries; the two 1 x 1 data gradients accumulate onto it
            nonlocal xbuf
            xbuf = buf
            call("danhip_residual_bwd", ptr(g), ptr(r), ptr(xmask), ptr(gr), ptr(buf), acc, g.numel(), stream())

        dx_ret = _deliver(xs, x.shape, x, skip_path) if need_dx else skip_path(None, 0)
        dhyper = torch.empty_like(hyper)
        dT = torch.empty_like(T)
        dU = torch.empty_like(U)
        grads = [None] * ctx.nw

        def sinks(i):
            wp, bp = ctx.handles[i]
            dw = db = None
            if ctx.needs_input_grad[5 + 2 * i] or ctx.blocks[i][0]:
                dw, grads[2 * i] = _grad_target(wp, ctx.khw[i] + (ctx.cin_real[i], ctx.couts[i]), dev)
            if ctx.needs_input_grad[6 + 2 * i] or ctx.blocks[i][1]:
                db, grads[2 * i + 1] = _grad_target(bp, (ctx.couts[i],), dev)
            return dw, db

        def dgrad(i, dyv, mask, dxv, acc):
            d = ctx.descs[i]
            pitch = _lib.ConvPitch(dyv.stride(2), dxv.stride(2), mask.stride(2) if mask is not None else 0)
            sc, nsc = _conv_scratch(d, 1, dev)
            e0 = _prof_begin()
            call("danhip_conv2d_bwd_data_strided", ctypes.byref(d), _vptr(dyv), ptr(wbs[i]), _vptr(mask) if mask is not None else None, _vptr(dxv), acc,
                 ctypes.byref(pitch), ptr(sc), nsc, stream())
            _prof_end(e0, d, 5 if mask is not None else 1)

        def wgrad(i, xv, dyv):
            dw, db = sinks(i)
            if dw is None:
                if db is not None:                               # (never in the reference graphs: a trainable bias comes with its kernel)
                    db.add_(dyv.to(torch.float32).sum((0, 1, 2)))
                return
            _wgrad_launch(ctx.descs[i], xv, dyv, dw, db, ctx.cin_real[i], (gr, dhyper, dT, dU))

        # residual conv: d hyper = (gr . W^T) * (hyper > 0); then every branch on its slice.  (The weight gradients of the two "plus" kernels
        # also fill the taps / columns their zeros occupy: FlatParams.mask_structured clears those before the optimizer, plain autograd
        # slices them away.)
        dgrad(5, gr, hyper, dhyper, 0)
        wgrad(5, hyper, gr)
        dgrad(4, dhyper[..., 192:256], U, dU, 0)
        wgrad(4, U, dhyper[..., 192:256])
        dgrad(3, dU, T[..., 64:128], dT[..., 64:128], 0)
        wgrad(3, T[..., 64:128], dU)
        dgrad(2, dhyper[..., 128:192], T[..., 0:64], dT[..., 0:64], 0)
        wgrad(2, T[..., 0:64], dhyper[..., 128:192])
        call("danhip_avgpool2x2s1_same_bwd_strided", _vptr(dhyper[..., 64:128]), 256, _vptr(dT[..., 128:192]), 192, N, H, W, 64, stream())
        if need_dx:
            dgrad(1, dT, xmask, xbuf, 1)
        wgrad(1, x, dT)
        if need_dx:
            dgrad(0, dhyper[..., 0:64], xmask, xbuf, 1)
        wgrad(0, x, dhyper[..., 0:64])
        if _CTX.GRAD_READY_HOOK is not None:
            for p_ in ctx.hook_order:                            # all of the block's gradients are issued: declare them in reverse creation order
                _CTX.GRAD_READY_HOOK(p_)
        return (dx_ret, None, None, None, None) + tuple(grads)


_CB_LAST = {}


def context_block(x, params, hook_order, trace_params=None):
    """params: six (w, b) pairs in the order b1, cat(b3 | b4 | b2), plus(b3a 3x1 | b3b 1x3) as a [3, 3, 64, 64] kernel, b43 (3x3), plus(b4a | b4b), res;
    hook_order: the block's kernel Parameters in reverse creation order (data-parallel gradient buckets); trace_params: {"b1", "b2", "b3",
    "b3a", "b3b", "b4", "b43", "b4a", "b4b", "res"} -> kernel Parameter (ops.TRACE: tests).  -> out (with a gradient slot)."""
    assert not _is_limbs(x), "context_block is a 16-bit training op (the nets take the unfused block on the fp32 / split paths)"
    track = torch.is_grad_enabled()
    handles, flat = [], []
    for w, b in params:
        handles.append((_param_handle(w), _param_handle(b)))
        flat += [w, b]
    yslot = _new_slot(track)
    out = _ContextBlock.apply(x, _slot_of(x) if (track and x.requires_grad) else None, yslot, handles, hook_order, *flat)
    if _CTX.TRACE is not None and trace_params:
        for k, prm in trace_params.items():
            _CTX.TRACE[id(prm)] = _CB_LAST[k].detach().contiguous()
        _CB_LAST.clear()
    return _publish(out, yslot, False)


class _ConcatMix(torch.autograd.Function):
    """out = relu([a | f] . Wv + bv) with a BLOCK-DIAGONAL Wv = diag(W1, W2): two 1x1 convolutions of two different maps written side by side
    into one map, i.e. concat([relu(conv1x1(a, W1)), relu(conv1x1(f, W2))]) — DAN's stage-2 input mix (net/danet.py:944-950), whose
    85 / 171 (170 / 342, 341 / 683) column counts fit no tile and went through the flat-M kernel plus torch.cat and, in backward, a slice
    pass per part — as ONE streaming GEMM over the never-materialised concatenation (danhip_conv2d_fwd_concat2) — round 4.
    `a` carries no gradient (the reference puts a stop_gradient on it).  Backward: the weight gradient of each input's [C, Co] row block by the
    ordinary 1x1 kernel against the FULL output gradient, after which the off-diagonal blocks (columns of the other part) are cleared;
    f's data gradient through the row block of f over all output columns (zeros where W1's columns are): dense 256-wide tiles, no ragged K."""

    @staticmethod
    def forward(ctx, a, f, fslot, yslot, handles, split, wv, bv):
        N, H, W, C1 = a.shape
        C2 = f.shape[-1]
        Co = wv.shape[3]
        dev = a.device
        assert a.dtype == ACT and f.dtype == ACT and a.is_contiguous() and f.is_contiguous() and a.shape[:3] == f.shape[:3]
        assert tuple(wv.shape[:3]) == (1, 1, C1 + C2) and wv.is_contiguous() and not a.requires_grad
        wvp, bvp, lowp = handles
        need_bwd = f.requires_grad or wv.requires_grad or bv.requires_grad or _sink_trainable(wv)
        d = _desc(N, H, W, C1 + C2, Co, 1, 1, 1)
        wf, _ = packed_weights(d, wv, wvp, False)
        out = torch.empty((N, H, W, Co), dtype=ACT, device=dev)
        e0 = _prof_begin()
        if C1 == C2 and _lib.lib().danhip_conv2d_fwd_concat2_supported(ctypes.byref(d), C1, C1):
            call("danhip_conv2d_fwd_concat2", ctypes.byref(d), ptr(a), ptr(f), C1, C1, ptr(wf), ptr(bv.detach()), ptr(out), 1, stream())
        else:                                            # small maps (the 20^2 .. 5^2 levels): concatenate, then the split-K / flat-M kernels
            x = torch.cat([a, f], dim=-1)
            ws, nws = _conv_scratch(d, 0, dev)
            call("danhip_conv2d_fwd_ws", ctypes.byref(d), ptr(x), ptr(wf), ptr(bv.detach()), ptr(out), BF16, 1, None, ptr(ws), nws, stream())
        _prof_end(e0, d, 0)
        ctx.dims = (N, H, W, C1, C2, Co)
        ctx.fslot, ctx.yslot, ctx.handles, ctx.split = fslot, yslot, handles, split
        ctx.set_materialize_grads(False)
        ctx.trainable = _sink_trainable(wv), _sink_trainable(bv)
        wb_low = None
        if need_bwd and f.requires_grad:
            d2 = _desc(N, H, W, C2, Co, 1, 1, 1)
            low = lowp if lowp is not None else wv[:, :, C1:, :]
            _, wb_low = packed_weights(d2, low, lowp, True)
        ctx.save_for_backward(a, f, out, wb_low)
        return out

    @staticmethod
    def backward(ctx, dy):
        a, f, out, wb_low = ctx.saved_tensors
        N, H, W, C1, C2, Co = ctx.dims
        dev = a.device
        M = N * H * W
        def prepare(dy):                                 # (slot deliveries are already multiplied by (out > 0); the autograd tensor is not)
            dy = dy.contiguous().clone()
            call("danhip_relu_bwd_bias_grad", ptr(dy), ptr(out), None, M, Co, stream())
            return dy

        g = _incoming(ctx.yslot, dy, prepare)
        if g is None:
            return (None,) * 8
        wvp, bvp, lowp = ctx.handles
        c1, o1 = ctx.split
        need_dw = ctx.needs_input_grad[6] or ctx.trainable[0]
        need_db = ctx.needs_input_grad[7] or ctx.trainable[1]
        # ---- f's data gradient first (it heads the critical path): dF = g . W[C1:, :]^T, delivered into f's slot (+ its ReLU backward)
        df = None
        if ctx.needs_input_grad[1]:
            d2 = _desc(N, H, W, C2, Co, 1, 1, 1)
            ws, nws = _conv_scratch(d2, 1, dev)
            e0 = _prof_begin()
            xs = ctx.fslot
            relu_f = xs is not None and xs.is_relu

            def data_grad(buf, acc):
                call("danhip_conv2d_bwd_data_ws", ctypes.byref(d2), ptr(g), ptr(wb_low), ptr(f) if relu_f else None, ptr(buf), acc, ptr(ws), nws, stream())

            df = _deliver(xs, f.shape, f, data_grad)
            _prof_end(e0, d2, 5 if relu_f else 1)
        dwv = dbv = None
        if need_dw:
            dw, dwv = _grad_target(wvp, (1, 1, C1 + C2, Co), dev)
            db = None
            if need_db:
                db, dbv = _grad_target(bvp, (Co,), dev)
            # row block of a (+ the bias gradient: column sums of g), row block of f; then the columns of the OTHER part go back to zero
            _wgrad_launch(_desc(N, H, W, C1, Co, 1, 1, 1), a, g, dw[:, :, :C1, :], db, C1, (g,))
            _wgrad_launch(_desc(N, H, W, C2, Co, 1, 1, 1), f, g, dw[:, :, C1:, :], None, C2, (g,))
            if c1 is not None:
                side = _CTX.wgrad["side"] if _CTX.wgrad["on"] else None
                with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
                    dw[:, :, :c1, o1:].zero_()
                    dw[:, :, c1:, :o1].zero_()
        elif need_db:
            raise NotImplementedError("a trainable bias without its kernel (no reference graph has one)")
        if _CTX.GRAD_READY_HOOK is not None and wvp is not None:
            _CTX.GRAD_READY_HOOK(wvp)
        return None, df, None, None, None, None, dwv, dbv


def concat_conv1x1_relu(a, f, wv, bv, split=None, trace_params=None):
    """relu(conv1x1(concat([a, f]), wv) + bv) without the concatenation; a is treated as a constant (stop_gradient).  wv: [1, 1, Ca + Cf, Co]
    (a FlatParams block-diagonal block, or any tensor); split = (rows, columns) of its upper-left block when wv is block-diagonal - the
    off-diagonal blocks of its gradient are then cleared.  trace_params: (w1, w2) kernel Parameters of the two parts (ops.TRACE: tests)."""
    assert not (_is_limbs(a) or _is_limbs(f)), "concat_conv1x1_relu is a 16-bit op (the nets take the unfused mix on the fp32 / split paths)"
    track = torch.is_grad_enabled() and (f.requires_grad or wv.requires_grad or _sink_trainable(wv))
    wvp, bvp = _param_handle(wv), _param_handle(bv)
    lowp = getattr(wv, "_danhip_lower", None)
    yslot = _new_slot(track)
    out = _ConcatMix.apply(a.detach(), f, _slot_of(f) if (track and f.requires_grad) else None, yslot, (wvp, bvp, lowp),
                           split if split is not None else (None, None), wv, bv)
    if _CTX.TRACE is not None and trace_params is not None and split is not None:
        _CTX.TRACE[id(trace_params[0])] = out.detach()[..., :split[1]].contiguous()
        _CTX.TRACE[id(trace_params[1])] = out.detach()[..., split[1]:].contiguous()
    return _publish(out, yslot, True)


class _BatchNorm(torch.autograd.Function):
    """tf.layers.batch_normalization(training=True) (+ optional ReLU) over NHWC bf16 — net/sfd_net.py:91-119."""

    @staticmethod
    def forward(ctx, x, gamma, beta, moving_mean, moving_var, eps, momentum, relu):
        C = x.shape[-1]
        M = x.numel() // C
        y = torch.empty_like(x)
        mean = torch.empty(C, dtype=torch.float32, device=x.device)
        rstd = torch.empty(C, dtype=torch.float32, device=x.device)
        ws = torch.empty(2 * C, dtype=torch.float64, device=x.device)      # sum x, sum x^2 in double
        call("danhip_batchnorm_fwd_train", ptr(x), ptr(gamma.detach()), ptr(beta.detach()), ptr(y), ptr(mean), ptr(rstd), ptr(moving_mean), ptr(moving_var),
             M, C, float(eps), float(momentum), int(relu), ptr(ws), stream())
        ctx.save_for_backward(x, gamma.detach(), mean, rstd, y if relu else None)
        ctx.relu = relu
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, rstd, y = ctx.saved_tensors
        C = x.shape[-1]
        M = x.numel() // C
        dy = dy.contiguous()
        if ctx.relu:
            dy = dy.clone()
            call("danhip_relu_bwd_bias_grad", ptr(dy), ptr(y), None, M, C, stream())
        dx = torch.empty_like(x)
        dgamma = torch.empty(C, dtype=torch.float32, device=x.device)
        dbeta = torch.empty(C, dtype=torch.float32, device=x.device)
        call("danhip_batchnorm_bwd", ptr(x), ptr(dy), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx), ptr(dgamma), ptr(dbeta), M, C, stream())
        return dx, dgamma, dbeta, None, None, None, None, None


def batch_norm_train(x, gamma, beta, moving_mean=None, moving_var=None, eps=1e-5, momentum=0.997, relu=False):
    assert not _is_limbs(x), "batch_norm_train: a 16-bit training op"
    return _BatchNorm.apply(x, gamma, beta, moving_mean, moving_var, eps, momentum, relu)


class _BatchNormFrozen(torch.autograd.Function):
    """tf.layers.batch_normalization(training=False) (+ optional ReLU) where a gradient is tracked (frozen statistics: freeze_bn, or a unit
    differentiated in inference mode): y = (x - mean) rstd gamma + beta with the moving statistics as constants, so dx = dy gamma rstd,
    dgamma = sum dy xhat, dbeta = sum dy.  Backward is two existing launches: danhip_batchnorm_bwd for the two sums (its dx, which
    subtracts the batch means of the training form, goes to a scratch tensor) and the apply kernel on dy with mean = beta = 0 for dx."""

    @staticmethod
    def forward(ctx, x, gamma, beta, mean, rstd, relu):
        C = x.shape[-1]
        x = x.contiguous()
        y = torch.empty_like(x)
        call("danhip_batchnorm_fwd_infer", ptr(x), ptr(gamma.detach()), ptr(beta.detach()), ptr(mean), ptr(rstd), ptr(y), x.numel() // C, C, int(relu), stream())
        ctx.save_for_backward(x, gamma.detach(), mean, rstd, y if relu else None)
        ctx.relu = relu
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, rstd, y = ctx.saved_tensors
        C = x.shape[-1]
        M = x.numel() // C
        dy = dy.contiguous()
        if ctx.relu:
            dy = dy.clone()
            call("danhip_relu_bwd_bias_grad", ptr(dy), ptr(y), None, M, C, stream())
        dx, unused = torch.empty_like(x), torch.empty_like(x)
        dgamma = torch.empty(C, dtype=torch.float32, device=x.device)
        dbeta = torch.empty(C, dtype=torch.float32, device=x.device)
        zero = torch.zeros(C, dtype=torch.float32, device=x.device)
        call("danhip_batchnorm_bwd", ptr(x), ptr(dy), ptr(gamma), ptr(mean), ptr(rstd), ptr(unused), ptr(dgamma), ptr(dbeta), M, C, stream())
        call("danhip_batchnorm_fwd_infer", ptr(dy), ptr(gamma), ptr(zero), ptr(zero), ptr(rstd), ptr(dx), M, C, 0, stream())
        return dx, dgamma, dbeta, None, None, None


def batch_norm_infer(x, gamma, beta, moving_mean, moving_var, eps=1e-5, relu=False):
    if torch.is_grad_enabled() and x.dtype == ACT and not _is_limbs(x) and (x.requires_grad or gamma.requires_grad or beta.requires_grad):
        # (without this the call below would cut the graph: nothing in front of a frozen batch norm received a gradient)
        return _BatchNormFrozen.apply(x, gamma, beta, moving_mean, torch.rsqrt(moving_var + eps), relu)
    x = _f32_in(x)
    C = x.shape[-1]
    y = torch.empty_like(x)
    rstd = torch.rsqrt(moving_var + eps)
    call("danhip_batchnorm_fwd_infer", ptr(x), ptr(gamma.detach()), ptr(beta.detach()), ptr(moving_mean), ptr(rstd), ptr(y), x.numel() // C, C, int(relu), stream())
    return y


class _BatchNormAct(torch.autograd.Function):
    """Batch norm (+ residual add) (+ ReLU) as ONE node on the fused tail kernels (csrc/bn_act.hip): y = act(xhat gamma + beta + shortcut),
    the tail of conv_bn / conv_bn_relu and of a bottleneck unit (net/resnet_danet.py:157-218).  frozen: the moving statistics are constants
    (training=False with a gradient tracked).  Backward is one library call - two launches - on dy as it comes: the ReLU mask [y > 0] is
    applied inside both passes, and the shortcut's gradient is written by the pass that writes dx."""

    @staticmethod
    def forward(ctx, x, shortcut, gamma, beta, moving_mean, moving_var, eps, momentum, relu, frozen):
        C = x.shape[-1]
        M = x.numel() // C
        y = torch.empty_like(x)
        if frozen:
            mean, rstd = moving_mean, torch.rsqrt(moving_var + eps)
            call("danhip_bn_act_fwd_infer", ptr(x), ptr(shortcut), ptr(gamma.detach()), ptr(beta.detach()), ptr(mean), ptr(rstd), ptr(y), M, C, int(relu),
                 stream())
        else:
            mean = torch.empty(C, dtype=torch.float32, device=x.device)
            rstd = torch.empty(C, dtype=torch.float32, device=x.device)
            ws = torch.empty(2 * C, dtype=torch.float64, device=x.device)      # sum x, sum x^2 in double
            call("danhip_bn_act_fwd_train", ptr(x), ptr(shortcut), ptr(gamma.detach()), ptr(beta.detach()), ptr(y), ptr(mean), ptr(rstd), ptr(moving_mean),
                 ptr(moving_var), M, C, float(eps), float(momentum), int(relu), ptr(ws), stream())
        ctx.save_for_backward(x, gamma.detach(), mean, rstd, y if relu else None)
        ctx.frozen, ctx.has_shortcut = frozen, shortcut is not None
        ctx.set_materialize_grads(False)
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return (None,) * 10
        x, gamma, mean, rstd, y = ctx.saved_tensors
        C = x.shape[-1]
        M = x.numel() // C
        dy = dy.contiguous()                                                # (no copy when it is)
        dx = torch.empty_like(x)
        dsc = torch.empty_like(x) if (ctx.has_shortcut and ctx.needs_input_grad[1]) else None
        sums = torch.empty((2, C), dtype=torch.float32, device=x.device)    # dgamma, dbeta side by side: one clear inside the call
        call("danhip_bn_act_bwd", ptr(x), ptr(dy), ptr(y), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx), ptr(dsc), ptr(sums[0]), ptr(sums[1]), M, C,
             int(ctx.frozen), stream())
        return dx, dsc, sums[0], sums[1], None, None, None, None, None, None


def _bn_act_fused(x, shortcut):
    """The fused tail takes 16-bit activations of the build's type (not fp32 tensors, not limb views: precision fp32 / split)."""
    return x.dtype == ACT and not _is_limbs(x) and (shortcut is None or (shortcut.dtype == ACT and not _is_limbs(shortcut)))


def _bn_act_unfused(y, shortcut, relu):
    if shortcut is not None:
        y = add(y, shortcut)
    return torch.relu(y) if relu and shortcut is not None else y


def batch_norm_act_train(x, gamma, beta, moving_mean=None, moving_var=None, eps=1e-5, momentum=0.997, relu=False, shortcut=None):
    """act(batch_norm(x, batch statistics) + shortcut) with the moving averages updated once: one autograd node, one apply pass forward,
    two launches backward.  A non-16-bit input takes the separate ops (batch_norm_train + add + ReLU)."""
    if not _bn_act_fused(x, shortcut):
        return _bn_act_unfused(batch_norm_train(x, gamma, beta, moving_mean, moving_var, eps, momentum, relu and shortcut is None), shortcut, relu)
    if shortcut is not None:
        assert shortcut.shape == x.shape, "batch_norm_act: the shortcut has the shape of x"
        shortcut = shortcut.contiguous()
    return _BatchNormAct.apply(x.contiguous(), shortcut, gamma, beta, moving_mean, moving_var, eps, momentum, bool(relu), False)


def batch_norm_act_infer(x, gamma, beta, moving_mean, moving_var, eps=1e-5, relu=False, shortcut=None):
    """The same with the moving statistics (training=False): one launch without a gradient, one autograd node with one.  A non-16-bit or
    limb input (precision fp32 / split) takes the separate ops (batch_norm_infer + add + ReLU)."""
    if not _bn_act_fused(x, shortcut):
        return _bn_act_unfused(batch_norm_infer(x, gamma, beta, moving_mean, moving_var, eps, relu and shortcut is None), shortcut, relu)
    if shortcut is not None:
        assert shortcut.shape == x.shape, "batch_norm_act: the shortcut has the shape of x"
        shortcut = shortcut.contiguous()
    return _BatchNormAct.apply(x.contiguous(), shortcut, gamma, beta, moving_mean, moving_var, eps, 0.0, bool(relu), True)


class _DeformSample(torch.autograd.Function):
    """Deformable im2col (cpp/Deform/deform_conv.cu:229-275) and its backward (col2im :281-328, col2im_coord :335-389):
    x bf16 [N,H,W,C], offsets bf16 [N,Ho,Wo,dg*2*kh*kw] -> S bf16 [N,Ho,Wo,kh*kw*C] (k = tap*C + c)."""

    @staticmethod
    def forward(ctx, x, offsets, kh, kw, stride, dilation, dg):
        N, H, W, C = x.shape
        Ho, Wo = -(-H // stride), -(-W // stride)
        assert x.dtype == ACT and offsets.dtype == ACT and x.is_contiguous() and offsets.is_contiguous()
        assert offsets.shape == (N, Ho, Wo, dg * 2 * kh * kw), (offsets.shape, (N, Ho, Wo, dg * 2 * kh * kw))
        S = torch.empty((N, Ho, Wo, kh * kw * C), dtype=ACT, device=x.device)
        call("danhip_deform_sample_fwd", ptr(x), ptr(offsets), ptr(S), N, H, W, C, kh, kw, stride, dilation, dg, stream())
        ctx.save_for_backward(x, offsets)
        ctx.cfg = (kh, kw, stride, dilation, dg)
        return S

    @staticmethod
    def backward(ctx, dS):
        x, offsets = ctx.saved_tensors
        kh, kw, stride, dilation, dg = ctx.cfg
        N, H, W, C = x.shape
        dx = torch.empty_like(x)
        doff = torch.empty_like(offsets)
        if _CTX.deterministic:      # + the ordered far-corner region (records, counts, starts); 0: the shape class has no ordered form
            nws = int(_lib.lib().danhip_deform_sample_bwd_ordered_workspace_bytes(N, H, W, C, dg))
            ws = torch.empty(max(nws // 4, x.numel() + 64), dtype=torch.float32, device=x.device)
        else:
            ws = torch.empty(x.numel() + 64, dtype=torch.float32, device=x.device)      # scatter target + the far-corner statistic
        call("danhip_deform_sample_bwd", ptr(x), ptr(offsets), ptr(dS.contiguous()), ptr(dx), ptr(doff), N, H, W, C, kh, kw, stride, dilation, dg, 0,
             ptr(ws), ws.numel() * 4, stream())
        return dx, doff, None, None, None, None, None


class _DeformConv(torch.autograd.Function):
    """DeformConvOp / DeformConvBackpropOp (cpp/Deform/deform_conv.cc:392-535, :635-771) through the single-call entry
    points.  KEEP_DEFORM_COL (default on): the forward's im2col buffer (9x the activation, 1.9 GB at 160x160x256 batch 16) is kept for
    the weight gradient instead of being re-sampled in backward as the reference does on its 11 GB cards (deform_conv.cc:744-748).
    x bf16 [N,H,W,C]; w fp32 [1,1,kh*kw*C,Cout] (the OIHW variable viewed as the GEMM operand); offsets bf16."""

    @staticmethod
    def forward(ctx, x, w, b, offsets, kh, kw, stride, dilation, dg, relu, b_param, yslot, xslot=None, w_param=None):
        N, H, W, C = x.shape
        cout = w.shape[-1]
        ctx.xslot = xslot
        ctx.w_param, ctx.block_w = w_param, _sink_trainable(w)
        assert x.dtype == ACT and offsets.dtype == ACT and x.is_contiguous() and offsets.is_contiguous()
        assert w.shape == (1, 1, kh * kw * C, cout) and cout % 8 == 0
        Ho, Wo = -(-H // stride), -(-W // stride)
        assert offsets.shape == (N, Ho, Wo, dg * 2 * kh * kw), (offsets.shape, (N, Ho, Wo, dg * 2 * kh * kw))
        d = _desc(N, Ho, Wo, kh * kw * C, cout, 1, 1, 1)
        need_bwd = w.requires_grad or x.requires_grad or offsets.requires_grad or ctx.block_w
        # (w_param: the GEMM operand is a block of the trainer's flat buffers or a cached gradient-free copy: packed once per weight version)
        wf, wb = packed_weights(d, w, w_param, need_bwd) if w_param is not None else pack_conv_weight(d, w.detach().contiguous(), need_bwd=need_bwd)
        y = torch.empty((N, Ho, Wo, cout), dtype=ACT, device=x.device)
        keep = _CTX.KEEP_DEFORM_COL and need_bwd
        if not keep and _lib.lib().danhip_deform_conv_fused(N, H, W, C, cout, kh, kw, stride, dg):
            ws, nws = None, 0                            # the fused kernel samples straight into the GEMM's LDS tile: no column buffer
        else:
            nws = _lib.lib().danhip_deform_conv_workspace_bytes(N, H, W, C, kh, kw, stride, 0)
            ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
        call("danhip_deform_conv_fwd", ptr(x), ptr(wf), ptr(b.detach()) if b is not None else None, ptr(offsets), ptr(y), N, H, W, C, cout, kh, kw,
             stride, dilation, dg, int(relu), ptr(ws) if ws is not None else None, nws, stream())
        ctx.cfg = (kh, kw, stride, dilation, dg, cout, relu)
        ctx.b_param, ctx.yslot, ctx.has_bias = b_param, yslot, b is not None
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, offsets, wb, y if relu else None)
        ctx.col = ws if keep else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, offsets, wb, y = ctx.saved_tensors
        kh, kw, stride, dilation, dg, cout, relu = ctx.cfg
        N, H, W, C = x.shape
        col, ctx.col = ctx.col, None
        def prepare(dy):                                 # (slot deliveries arrive ReLU-masked; the autograd tensor does not)
            assert dy.dtype == ACT and dy.shape[-1] == cout
            dy = dy.contiguous()
            if relu:
                dy = dy.clone()
                call("danhip_relu_bwd_bias_grad", ptr(dy), ptr(y), None, dy.numel() // cout, cout, stream())
            return dy

        g = _incoming(ctx.yslot, dy, prepare)
        if g is None:
            return (None,) * 14
        bp = ctx.b_param
        db, db_ret = _grad_target(bp, (cout,), x.device) if (ctx.has_bias and ctx.needs_input_grad[2]) else (None, None)
        dw, dw_ret = _grad_target(ctx.w_param, (1, 1, kh * kw * C, cout), x.device)       # (a sink: the flat gradient buffer's block)
        doff = torch.empty_like(offsets)
        nws = _lib.lib().danhip_deform_conv_workspace_bytes(N, H, W, C, kh, kw, stride, 1)
        if _CTX.deterministic:      # + the ordered far-corner region and the weight gradient's partial rows; 0 (the call then raises): no ordered form
            nws = int(_lib.lib().danhip_deform_conv_bwd_ordered_workspace_bytes(N, H, W, C, cout, kh, kw, stride, dg)) or nws
        ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
        # x's gradient goes straight into its producer's slot - times (x > 0) when x is a ReLU output, added to what other consumers (the
        # offset convolution) delivered - instead of through an autograd tensor the producer would clone, mask and add (three map-sized passes)
        xs = ctx.xslot if ctx.needs_input_grad[0] else None

        def launch(dx, acc):
            call("danhip_deform_conv_bwd_deliver", ptr(x), ptr(wb), ptr(offsets), ptr(g), ptr(col), ptr(dx), ptr(doff), ptr(dw), ptr(db), N, H, W, C, cout,
                 kh, kw, stride, dilation, dg, acc, 1 if (xs is not None and xs.is_relu) else 0, ptr(ws), nws, stream())

        dx = _deliver(xs, x.shape, x, launch)
        if _CTX.GRAD_READY_HOOK is not None and bp is not None:
            _CTX.GRAD_READY_HOOK(bp)
        if _CTX.GRAD_READY_HOOK is not None and dw_ret is None:
            _CTX.GRAD_READY_HOOK(ctx.w_param)
        return (dx, dw_ret, db_ret, doff) + (None,) * 10


def deform_conv(x, w1x1, b, offsets, kh, kw, stride=1, dilation=1, deformable_group=1, relu=False):
    """y = act(DeformConvOp(x, filter, offsets) + b); w1x1 = the filter viewed [1,1,kh*kw*C,Cout]."""
    x, offsets = _f32_in(x, offsets)
    if _f32_infer(x):
        N, H, W, C = x.shape
        Ho, Wo = -(-H // stride), -(-W // stride)
        S = torch.empty((N, Ho, Wo, kh * kw * C), dtype=torch.float32, device=x.device)
        call("danhip_deform_sample_fwd_f32", ptr(x.contiguous()), ptr(offsets.contiguous()), ptr(S), N, H, W, C, kh, kw, stride, dilation, deformable_group,
             stream())
        return (_conv2d_split if _CTX.SPLIT_EVAL else _conv2d_f32)(S, w1x1, b, 1, relu, None, "same")
    bp = b if isinstance(b, torch.nn.Parameter) else None
    wp = w1x1 if hasattr(w1x1, "_danhip_grad") else None
    track = torch.is_grad_enabled() and (x.requires_grad or w1x1.requires_grad or offsets.requires_grad or _sink_trainable(w1x1))
    yslot = _new_slot(track)
    y = _DeformConv.apply(x, w1x1, b, offsets, kh, kw, stride, dilation, deformable_group, relu, bp, yslot,
                          _slot_of(x) if (track and x.requires_grad) else None, wp)
    return _publish(y, yslot, relu)


def preprocess_f32(img_rgb_u8):
    """uint8 RGB [N,H,W,3] -> fp32 [N,H,W,3] BGR - mean (dan_preprocessing.py:55-57,755-758): exact fp32 subtraction, 3 real channels."""
    assert img_rgb_u8.dtype == torch.uint8 and img_rgb_u8.shape[-1] == 3
    means = torch.tensor([123.68, 116.78, 103.94], dtype=torch.float32, device=img_rgb_u8.device)
    return (img_rgb_u8.to(torch.float32) - means).flip(-1).contiguous()


def deform_sample(x, offsets, kh, kw, stride=1, dilation=1, deformable_group=1):
    x, offsets = _f32_in(x, offsets)
    return _DeformSample.apply(x, offsets, kh, kw, stride, dilation, deformable_group)


def face_scores(cls, threshold=None):
    """softmax(cls)[..., 1] of two-way fp32 logits [..., 2] (eval_dan.py:356, eval_sfd.py:281) -> scores [...]; with `threshold` also the int32
    mask (score > threshold) (train_dan.py:438-439): -> (scores, mask).  One libdanhip launch (no torch.softmax on the product path)."""
    assert cls.dtype == torch.float32 and cls.shape[-1] == 2
    c = cls.contiguous()
    n = c.numel() // 2
    score = torch.empty(c.shape[:-1], dtype=torch.float32, device=c.device)
    mask = torch.empty(c.shape[:-1], dtype=torch.int32, device=c.device) if threshold is not None else None
    call("danhip_face_scores", ptr(c), ptr(score), ptr(mask), float(threshold or 0.0), n, stream())
    return (score, mask) if threshold is not None else score


def argsort_desc(scores, ties_high_index_first=False):
    """Positions of a 1-D fp32 vector by descending value, equal values by ascending index — torch.sort(descending=True, stable=True).indices,
    i.e. tf.nn.top_k's / tf.image.non_max_suppression's candidate order (utility/bbox_util.py:61-91); ties_high_index_first: numpy's
    argsort()[::-1] (eval_dan.py:255).  -> int64 indices.  libdanhip's bitonic arg-sort (csrc/sort.hip): no torch.sort on the product path."""
    assert scores.dim() == 1 and scores.dtype == torch.float32
    n = scores.shape[0]
    idx = torch.empty((n,), dtype=torch.int32, device=scores.device)
    if n == 0:
        return idx.long()
    s = scores.contiguous()
    nbytes = int(_lib.lib().danhip_argsort_workspace_bytes(n))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=scores.device)
    call("danhip_argsort_desc_f32", ptr(s), n, 1 if ties_high_index_first else 0, ptr(idx), ptr(ws), nbytes, stream())
    return idx.long()


# ---- `ops.USE_SLOTS`, `ops.TRACE = {}` ... (rounds 1-4 spelling; tests, bench.py, tools): reads and writes go to the active context
class _OpsModule(type(os)):
    def __getattr__(self, name):
        if name in _CTX_FIELDS:
            return getattr(_CTX, name)
        raise AttributeError("module %r has no attribute %r" % (self.__name__, name))

    def __setattr__(self, name, value):
        if name in _CTX_FIELDS:
            setattr(_CTX, name, value)
        else:
            super().__setattr__(name, value)


import sys as _sys  # noqa: E402
_sys.modules[__name__].__class__ = _OpsModule
