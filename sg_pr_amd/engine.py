"""ctypes binding of the C-ABI in include/sgpr.h (libsgpr_hip.so) + weight-blob packing.

This is the only place the Python host touches the HIP engine.  PyTorch is used
for device memory and streams only: tensors are handed over as raw pointers.
There is NO CPU fallback: a missing library or a non-GPU tensor raises.
"""
import ctypes
import functools
import os
from fractions import Fraction
import threading

import numpy as np
import torch

from . import _build

# include/sgpr.h is the one declaration of the C-ABI: its functions, limits, flag bits and error codes are read from it
_ABI = _build.header_abi()
_C = _ABI.constants

NUM_LABELS = 12
F3 = 32
MAX_NODES = _C["SGPR_MAX_NODES"]     # node_num of the tuned kernels (beyond: the any-shape kernels)

# order of the fp32 tensors in the weights blob (include/sgpr.h, sgpr_weights_count)
_CONV_BLOCKS = ["dgcnn_s_conv1", "dgcnn_f_conv1", "dgcnn_s_conv2", "dgcnn_f_conv2",
                "dgcnn_s_conv3", "dgcnn_f_conv3", "dgcnn_conv_end"]
BLOB_KEYS = []
for _b in _CONV_BLOCKS:
    BLOB_KEYS += [_b + ".0.weight", _b + ".1.weight", _b + ".1.bias", _b + ".1.running_mean", _b + ".1.running_var"]
BLOB_KEYS += ["attention.weight_matrix", "tensor_network.weight_matrix", "tensor_network.weight_matrix_block",
              "tensor_network.bias", "fully_connected_first.weight", "fully_connected_first.bias",
              "scoring_layer.weight", "scoring_layer.bias"]

SGPR_OK = _ABI.errors["SGPR_OK"]
ERROR_NAMES = {code: name for name, code in _ABI.errors.items() if code != SGPR_OK}

# every symbol include/sgpr.h declares (tests check the library exports all of them)
ABI_SYMBOLS = [name for name, _, _ in _ABI.functions]


# struct sgpr_rank_group of include/sgpr.h
RANK_GROUP = np.dtype([("value", "<f4", (8,)), ("pairs", "<u4", (8,))])


SEQ_MAX_PATHS = _C["SGPR_SEQ_MAX_PATHS"]
SEQ_PATH_MAX_OFFSET = _C["SGPR_SEQ_PATH_MAX_OFFSET"]


def _slope(s):
    """(p, q) of a slope given as a pair, a Fraction, an int or a string like "3/2"; p >= 0, q >= 1, in lowest terms"""
    if isinstance(s, str):
        s = Fraction(s.strip())
    elif isinstance(s, (tuple, list)):
        if len(s) != 2:
            raise ValueError("a slope pair is (p, q), got %r" % (s,))
        s = Fraction(int(s[0]), int(s[1]))
    else:
        s = Fraction(s)
    if s < 0:
        raise ValueError("a slope must not be negative, got %s" % s)
    return s.numerator, s.denominator


def seq_paths(seq_len, slopes):
    """The path table of Engine.seq_path_filter / score_path_topk for a set of slopes: int32 [P, seq_len].
    A slope p/q (a (p, q) pair, a Fraction or a string like "3/2") means p columns per q rows; it gives one path per
    phase j in 0..q-1, off[d] = (d p + j) // q.  Paths are de-duplicated in order.  ValueError past SEQ_MAX_PATHS paths
    or past offset SEQ_PATH_MAX_OFFSET."""
    seq_len = int(seq_len)
    if seq_len < 1 or seq_len > Engine.SEQ_MAX_LEN:
        raise ValueError("seq_len must lie in 1..%d, got %d" % (Engine.SEQ_MAX_LEN, seq_len))
    paths = []
    for s in slopes:
        p, q = _slope(s)
        for j in range(q):
            off = tuple((d * p + j) // q for d in range(seq_len))
            if off[-1] > SEQ_PATH_MAX_OFFSET:
                raise ValueError("slope %d/%d walks %d columns back in %d scans: more than %d"
                                 % (p, q, off[-1], seq_len, SEQ_PATH_MAX_OFFSET))
            if off not in paths:
                paths.append(off)
    if not paths:
        raise ValueError("no slopes given")
    if len(paths) > SEQ_MAX_PATHS:
        raise ValueError("%d distinct paths: more than %d" % (len(paths), SEQ_MAX_PATHS))
    return np.asarray(paths, dtype=np.int32).reshape(len(paths), seq_len)


def _path_table(paths, seq_len):
    """a host int32 [P, seq_len] C-contiguous array of a path table (the library checks its contents)"""
    if isinstance(paths, torch.Tensor):
        paths = paths.cpu().numpy()
    t = np.ascontiguousarray(np.asarray(paths, dtype=np.int32))
    if t.ndim != 2 or t.shape[1] != int(seq_len):
        raise ValueError("paths must be [P, %d], got %s" % (int(seq_len), tuple(t.shape)))
    return t


SESSION_MAX = _C["SGPR_SESSION_MAX"]


def _session_table(starts):
    """a host int32 C-contiguous array of session starts, or None (the library checks its contents)"""
    if starts is None:
        return None
    if isinstance(starts, torch.Tensor):
        starts = starts.cpu().numpy()
    t = np.ascontiguousarray(np.asarray(starts, dtype=np.int32))
    if t.ndim != 1 or t.shape[0] < 1:
        raise ValueError("a session table is a 1-d array of at least one start, got shape %s" % (tuple(t.shape),))
    return t


def _table_args(t):
    """(pointer, n) of an optional host table (_session_table, _path_table) as the C-ABI takes it; None: (NULL, 0)"""
    return (None, 0) if t is None else (t.ctypes.data, t.shape[0])


class SgprError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("%s (%d): %s" % (ERROR_NAMES.get(code, "SGPR_E_?"), code, message))
        self.code = code


class SgprPairsJob(ctypes.Structure):
    """struct sgpr_pairs_job of include/sgpr.h"""
    _fields_ = [("d_pooled_rows", ctypes.c_void_p), ("R", ctypes.c_int32), ("d_pooled_cols", ctypes.c_void_p),
                ("M", ctypes.c_int32), ("d_score", ctypes.c_void_p), ("ld", ctypes.c_int64)]


class SgprDims(ctypes.Structure):
    _fields_ = [("num_labels", ctypes.c_int32), ("filters_1", ctypes.c_int32), ("filters_2", ctypes.c_int32),
                ("filters_3", ctypes.c_int32), ("tensor_neurons", ctypes.c_int32),
                ("bottle_neck_neurons", ctypes.c_int32)]


_lib = None


def load_library():
    """dlopen libsgpr_hip.so (built in-tree by sg_pr_amd._build / __graft_entry__.build)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("SGPR_HIP_LIB") or _build.LIB_PATH   # override: an alternative build of the same C-ABI
    if not os.path.exists(path):
        raise ImportError("HIP engine %s is not built; run `python -m sg_pr_amd._build` "
                          "(there is no CPU fallback)" % path)
    lib = ctypes.CDLL(path)
    # first thing: a library built from other sources than the header this binding follows must say so before any
    # missing symbol raises an AttributeError
    want = _build.header_abi_version()
    try:
        lib.sgpr_abi_version.restype = ctypes.c_int
        lib.sgpr_abi_version.argtypes = []
        have = lib.sgpr_abi_version()
    except AttributeError:
        have = None
    if have != want:
        raise ImportError("%s reports C-ABI version %s, include/sgpr.h declares %d: rebuild it "
                          "(`python -m sg_pr_amd._build --force`)" % (path, have, want))
    # the signatures are the header's (_build.parse_header): there is no table of them in Python
    for name, restype, argtypes in _ABI.functions:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


@functools.lru_cache(maxsize=None)
def public_header(file_name):
    """_build.parse_header of include/<file_name>: what one of the further public headers declares (needs no library)"""
    with open(os.path.join(_build.REPO, "include", file_name)) as f:
        return _build.parse_header(f.read())


@functools.lru_cache(maxsize=None)
def bind_header(file_name):
    """public_header(file_name) with its functions' signatures set on the one library load_library() returns -> the
    HeaderAbi.  A library that lacks one of the functions was built from other sources: ImportError."""
    abi, lib = public_header(file_name), load_library()
    for name, restype, argtypes in abi.functions:
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise ImportError("%s does not export %s: rebuild it (`python -m sg_pr_amd._build --force`)"
                              % (_build.LIB_PATH, name))
        fn.restype, fn.argtypes = restype, argtypes
    return abi


def default_dims():
    return SgprDims(NUM_LABELS, 64, 64, 32, 16, 16)


def dims_from_args(args, number_of_labels=NUM_LABELS):
    return SgprDims(int(number_of_labels), int(args.filters_1), int(args.filters_2), int(args.filters_3),
                    int(args.tensor_neurons), int(args.bottle_neck_neurons))


def blob_from_state_dict(sd):
    """Flatten a reference state dict (with or without the `module.` prefix) into the fp32 blob."""
    parts = []
    for key in BLOB_KEYS:
        t = sd[key] if key in sd else sd["module." + key]
        parts.append(t.detach().to(torch.float32).cpu().contiguous().view(-1).numpy())
    return np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


_UNSET = object()      # "argument not passed" where None is a value


def _check(rc):
    if rc != SGPR_OK:
        raise SgprError(rc, load_library().sgpr_last_error().decode())


def _stream(device):
    """the stream current on `device`, as the C-ABI takes it"""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _device_of(*tensors):
    """the device of the first CUDA tensor among the arguments, else the current device"""
    return next((t.device for t in tensors if isinstance(t, torch.Tensor) and t.is_cuda),
                torch.device("cuda", torch.cuda.current_device()))


def _on(t, device, dtype):
    """t (a tensor or anything torch.as_tensor takes) on `device`, of `dtype`, contiguous; as it is where it is all that"""
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t)
    if t.device != device or t.dtype != dtype or not t.is_contiguous():
        t = t.to(device=device, dtype=dtype).contiguous()
    return t


class Engine:
    """One packed-weights handle on one GPU (immutable after creation)."""

    def __init__(self, state_dict, dims=None, device=0):
        self._h = None
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise RuntimeError("sg_pr_amd.Engine needs a ROCm GPU (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
        self.device = torch.device("cuda", int(device) if not isinstance(device, torch.device) else device.index or 0)
        self.dims = dims if dims is not None else default_dims()
        # The tuned kernels run on the built shapes (32 pooled features, 12 label channels ...); a smaller architecture is
        # served by zero-padding its tensors at sgpr_create.  Device buffers keep the built widths (pooled [G, 32]: the
        # channels the checkpoint does not have are exactly 0); node embeddings are cut to filters_3 where they leave the
        # engine.  A larger architecture gets an any-shape handle (plain-fp32 kernels, buffers of the model's own width).
        self.f3 = int(self.dims.filters_3)
        self.pw = F3                                                     # floats per pooled / emb row (set below)
        self.any_shape = False
        if isinstance(state_dict, (np.ndarray, torch.Tensor)):          # already the flat fp32 blob (sg_pr_amd.ops)
            blob = np.ascontiguousarray(torch.as_tensor(state_dict).detach().cpu().numpy(), dtype=np.float32).ravel()
        else:
            blob = blob_from_state_dict(state_dict)
        want = self.lib.sgpr_weights_count(ctypes.byref(self.dims))
        h = ctypes.c_void_p()
        rc = self.lib.sgpr_create(blob.ctypes.data_as(ctypes.c_void_p), blob.size, ctypes.byref(self.dims),
                                  self.device.index, ctypes.byref(h))
        self._check(rc)
        assert want == blob.size
        self._h = h
        self.pw = int(self.lib.sgpr_pooled_width(h))
        self.any_shape = bool(self.lib.sgpr_is_any_shape(h))
        self.num_cus = int(torch.cuda.get_device_properties(self.device).multi_processor_count)
        self._order_cache = []            # (tensor objects, offsets, shape, versions, K) -> device launch order + node_cap, see embed()
        self._order_lock = threading.Lock()
        self._host_bufs = threading.local()  # per-thread pinned read-back buffers (f1_max)

    def close(self):
        if self._h is not None:
            self.lib.sgpr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    _check = staticmethod(_check)

    def _stream(self):
        return _stream(self.device)

    def _dev(self, t, dtype, name):
        return _on(t, self.device, dtype)

    def _pooled(self, t, name):
        """a pooled-vector argument on the device, fp32, contiguous - and of THIS handle's row width: the kernels read
        row r at p + r * width, so rows of another engine (or a [:, :filters_3] cut) would be read past their end"""
        t = self._dev(t, torch.float32, name)
        if t.dim() != 2 or t.shape[1] != self.pw:
            raise ValueError("%s must be [rows, %d] (this handle's pooled width), got %s" % (name, self.pw, tuple(t.shape)))
        return t

    def _cut(self, emb):
        """node embeddings [.., pooled width] -> [.., filters_3] (a view; identity for the shipped architecture)"""
        return emb if emb is None or self.f3 == self.pw else emb[..., :self.f3]

    def _ws(self, nbytes):
        return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=self.device)

    def lds_bytes(self, node_num, k):
        return int(self.lib.sgpr_embed_lds_bytes(self._h, node_num, k))

    PHASES = ["stage", "select", "gram", "gemm", "-", "gather", "conv_end", "attention"]

    def phase_profile(self, centers, labels, k, reps=3, node_cap=0, order=None, select_split=False):
        """Debug: workgroup cycles per phase of the embed kernel (thread-0 clocks at the barriers, on the profile
        instance of the kernel).  select_split adds timers inside the selection (they perturb it)."""
        buf = torch.zeros(16, dtype=torch.int64, device=self.device)
        self.lib.sgpr_debug_set_profile_buffer(self._h, _ptr(buf))
        self.lib.sgpr_debug_set_skip_mask(self._h, 128 if select_split else 0)
        try:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                self.embed(centers, labels, k, node_cap=node_cap, order=order)
            e1.record()
            torch.cuda.synchronize(self.device)
            self.last_profile_ms = e0.elapsed_time(e1) / reps     # launch time WITH the timers running
        finally:
            self.lib.sgpr_debug_set_profile_buffer(self._h, None)
            self.lib.sgpr_debug_set_skip_mask(self._h, 0)
        call = buf.cpu().numpy().astype(np.float64)
        self.last_select_split = call[8:14]   # load, sort, merge, tau+masks, prefix, emit (thread-0 cycles)
        c = call[:8]
        return dict(zip(self.PHASES, c / max(c.sum(), 1.0))), c

    def check_status(self):
        """Synchronises the stream and raises SgprError if a launch since the last check saw a label outside
        [-1, num_labels) (the reference raises KeyError, sg_net.py:277) or a graph that broke its node_cap promise."""
        self._check(self.lib.sgpr_check_status(self._h, self._stream()))

    def uses_f16_planes(self):
        """True: the default two-plane f16 datapath serves this checkpoint; False: the wide-range instance throughout."""
        return bool(self.lib.sgpr_debug_uses_f16_planes(self._h))

    def set_skip_mask(self, mask):
        """Debug / ablation only (include/sgpr.h)."""
        self.lib.sgpr_debug_set_skip_mask(self._h, int(mask))

    # ------------------------------------------------------------------ per-graph half
    @staticmethod
    def processed_slots(centers, labels, k):
        """Slots the kernel processes per graph, int64 [G] (see sgpr_embed_capped): trailing slots identical to the
        last one collapse to one representative when there are >= k of them.  numpy arrays or tensors."""
        c = torch.as_tensor(centers)
        l = torch.as_tensor(labels)
        n = l.shape[1]
        same = (l == l[:, -1:]) & (c == c[:, -1:, :]).all(-1)
        idx = torch.arange(n, device=l.device).expand_as(l)
        nd = torch.where(~same, idx + 1, torch.zeros_like(idx)).amax(dim=1)          # slots before the trailing run
        m = n - nd
        return nd + torch.where((m >= k) & (m > 1), torch.ones_like(m), m)

    @staticmethod
    def node_cap_of(centers, labels, k):
        """Largest number of slots the kernel will process for any graph of the batch.
        For device tensors this synchronises (do it once per dataset)."""
        eff = Engine.processed_slots(centers, labels, k)
        return int(eff.max().item()) if eff.numel() else 0

    def size_order(self, centers, labels, k):
        """Launch order for sgpr_embed_ordered: graph indices sorted by processed slots, largest first (stable), plus
        the node_cap they justify -> (order i32 device tensor [G], node_cap).  A property of the packed data - build
        it once per dataset.  Computed on the device (sgpr_size_order: two small launches and a 4-byte read-back, which
        synchronises); host arrays are uploaded first.  Beyond the tuned kernels' node_num / on an any-shape handle
        (where no launch takes a node_cap) the torch form below answers."""
        labels_t = torch.as_tensor(labels)
        g, n = labels_t.shape
        if g == 0:
            return torch.empty(0, dtype=torch.int32, device=self.device), 0
        if n > MAX_NODES or self.any_shape:
            return self.size_order_torch(centers, labels, k)
        order, info = self.size_order_device(self._dev(centers, torch.float32, "centers"),
                                             self._dev(labels_t, torch.int32, "labels"), None, n, k)
        return order, int(info[0].item())

    def size_order_torch(self, centers, labels, k):
        """size_order by torch ops (the checker of the device kernel; any node_num)."""
        eff = self.processed_slots(centers, labels, k)
        if eff.numel() == 0:
            return torch.empty(0, dtype=torch.int32, device=self.device), 0
        order = torch.argsort(eff, descending=True, stable=True).to(torch.int32).to(self.device)
        return order, int(eff.max().item())

    def size_order_device(self, centers, labels, offsets, node_num, k):
        """sgpr_size_order without the read-back: (order i32 [G], info i32 [2] = node_cap, graphs beyond 64 slots), both
        on the device, asynchronous.  Padded arrays (offsets None) or a ragged store's offsets (centers / labels None)."""
        g = (offsets.numel() - 1) if offsets is not None else labels.shape[0]
        order = torch.empty(g, dtype=torch.int32, device=self.device)
        info = torch.empty(2, dtype=torch.int32, device=self.device)      # (both entries are written by the kernel)
        ws_bytes = self.lib.sgpr_size_order_workspace_bytes(g)
        ws = self._ws(ws_bytes)
        rc = self.lib.sgpr_size_order(self._h, _ptr(centers if offsets is None else None),
                                      _ptr(labels if offsets is None else None), _ptr(offsets), g, int(node_num), int(k),
                                      _ptr(order), _ptr(info), _ptr(ws), ws_bytes, self._stream())
        self._check(rc)
        return order, info

    def _cached_order(self, centers, labels, k):
        """The largest-first launch order and the node_cap of a RESIDENT batch (sgpr_size_order, asynchronous), remembered per
        tensor pair, so that evaluating the same packed store again costs nothing -> (order, node_cap or 0).  An entry
        belongs to the tensors' base OBJECTS (weak references: a new tensor that happens to reuse the address of a freed
        one is a different object), their storage offsets / shapes, torch's in-place version counters and K.  Inference
        tensors (torch.inference_mode) have no version counter: their entry is kept by object, offsets, shape and K alone.
        The node_cap travels to pinned host memory behind an event and is returned from the first later call that finds
        the copy complete (no synchronisation, ever); embed() does not promise it (see there).  The order is made on the
        stream current at the first call: a hit on another stream waits for that event and records the order on its own
        stream.  A stale order is harmless - it is a permutation of the batch's graphs and decides when a graph runs,
        never what it yields.  A data-set property kept by the binding (under a lock: one Engine serves several threads);
        the C-ABI stays stateless."""
        import weakref
        bc = centers._base if centers._base is not None else centers
        bl = labels._base if labels._base is not None else labels
        tracked = not (centers.is_inference() or labels.is_inference())
        versions = (centers._version, labels._version) if tracked else (None, None)
        key = (centers.storage_offset(), labels.storage_offset(), tuple(labels.shape)) + versions + (int(k),)
        cur = torch.cuda.current_stream(self.device)
        with self._order_lock:
            live = []
            hit = None
            for entry in self._order_cache:
                rc, rl, kk, order, info_h, ev, made_on = entry
                if rc() is None or rl() is None:
                    continue                                   # a tensor of the entry is gone
                live.append(entry)
                if kk == key and rc() is bc and rl() is bl:
                    hit = entry
            self._order_cache = live
            if hit is not None:
                _, _, _, order, info_h, ev, made_on = hit
                if made_on != cur:
                    cur.wait_event(ev)                         # the order is complete before this stream reads it ...
                    order.record_stream(cur)                   # ... and its memory is not reused while it may
                return order, int(info_h[0]) if ev.query() else 0
            order, info = self.size_order_device(centers, labels, None, labels.shape[1], k)
            info_h = torch.empty(2, dtype=torch.int32).pin_memory()
            info_h.copy_(info, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(cur)
            self._order_cache = self._order_cache[-7:] + [(weakref.ref(bc), weakref.ref(bl), key, order, info_h, ev, cur)]
            return order, 0

    def embed(self, centers, labels, k, want_att=False, want_emb=False, debug=False, node_cap=0, order=None, auto_order=True):
        """centers [G,N,3] f32, labels [G,N] i32 (-1 = pad) -> pooled [G,32] (+ att [G,N], emb [G,N,32]).
        node_cap: optional promise on the processed slots per graph (node_cap_of); 0 = none.
        order: optional i32 launch order (size_order) - graphs not listed keep uninitialised output rows.
        auto_order: no order given and the arrays already resident on this device (more graphs than CUs, the tuned kernels'
        node_num): launch in the largest-first order sgpr_size_order makes on the device, computed once per tensor pair
        (_cached_order) - same bits, faster than storage order on KITTI-like data; False = the plain C-ABI call.  The
        cached node_cap is NOT promised: a write torch does not track (`x.data.copy_`, DLPack, a kernel writing through
        data_ptr()) leaves the cache key as it was, and a promise made from it could be broken by the data (NaN +
        SGPR_E_NODES).  Callers who know their data pass node_cap= themselves (size_order gives it)."""
        resident = (isinstance(centers, torch.Tensor) and isinstance(labels, torch.Tensor) and centers.device == self.device
                    and labels.device == self.device and centers.dtype == torch.float32 and labels.dtype == torch.int32
                    and centers.is_contiguous() and labels.is_contiguous())
        centers = self._dev(centers, torch.float32, "centers")
        labels = self._dev(labels, torch.int32, "labels")
        g, n = labels.shape
        assert centers.shape == (g, n, 3), "centers must be [G, N, 3]"
        if (order is None and auto_order and resident and not debug and g > self.num_cus and n <= MAX_NODES and k <= n
                and not self.any_shape):
            order = self._cached_order(centers, labels, k)[0]
        pooled = torch.empty(g, self.pw, dtype=torch.float32, device=self.device)
        att = torch.empty(g, n, dtype=torch.float32, device=self.device) if (want_att or debug) else None
        emb = torch.empty(g, n, self.pw, dtype=torch.float32, device=self.device) if (want_emb or debug) else None
        ws_bytes = self.lib.sgpr_embed_workspace_bytes(self._h, g, n, k)
        ws = self._ws(ws_bytes)
        if debug:
            layers = torch.zeros(g, 6, n, 64, dtype=torch.float32, device=self.device)
            knn = torch.full((g, 6, n, k), -1, dtype=torch.int32, device=self.device)
            rc = self.lib.sgpr_embed_debug(self._h, _ptr(centers), _ptr(labels), g, n, k, _ptr(pooled), _ptr(att),
                                           _ptr(emb), _ptr(layers), _ptr(knn), _ptr(ws), ws_bytes, self._stream())
            self._check(rc)
            return pooled, att, self._cut(emb), layers, knn
        if g == 0:
            return pooled, att, self._cut(emb)
        if order is not None:
            order = self._dev(order, torch.int32, "order")
            rc = self.lib.sgpr_embed_ordered(self._h, _ptr(centers), _ptr(labels), g, n, int(node_cap), k, _ptr(order),
                                             order.numel(), _ptr(pooled), _ptr(att), _ptr(emb), _ptr(ws), ws_bytes,
                                             self._stream())
            self._check(rc)
            return pooled, att, self._cut(emb)
        rc = self.lib.sgpr_embed_capped(self._h, _ptr(centers), _ptr(labels), g, n, int(node_cap), k, _ptr(pooled),
                                        _ptr(att), _ptr(emb), _ptr(ws), ws_bytes, self._stream())
        self._check(rc)
        return pooled, att, self._cut(emb)

    @staticmethod
    def to_ragged(centers, labels, num_labels=NUM_LABELS):
        """Padded arrays (centers [G,N,3], labels [G,N], -1 = pad, padding trailing) -> the ragged store of
        sgpr_embed_ragged: (centers f32 [S,3], labels i8 [S], offsets i64 [G+1]) as numpy arrays."""
        import numpy as np
        c = np.asarray(centers, dtype=np.float32)
        l = np.asarray(labels)
        real = l >= 0
        if real.any() and int(l[real].max()) >= num_labels:
            # an int8 cast would wrap 256 + c into the valid class c: refuse like the padded path and the reference do
            # (KeyError, sg_net.py:277)
            raise ValueError("to_ragged: label %d outside [0, %d)" % (int(l[real].max()), num_labels))
        counts = real.sum(1)
        if not (real == (np.arange(l.shape[1])[None, :] < counts[:, None])).all():
            raise ValueError("to_ragged: padding slots (label -1) must trail the real nodes of every graph")
        offsets = np.zeros(l.shape[0] + 1, dtype=np.int64)
        np.cumsum(counts, out=offsets[1:])
        return np.ascontiguousarray(c[real]), np.ascontiguousarray(l[real].astype(np.int8)), offsets

    @staticmethod
    def ragged_blob(centers, labels, offsets, pin=True):
        """The ragged store as ONE host buffer (offsets | centers | labels, each part 16-byte aligned): one H2D copy
        instead of three (each copy has its own ~10 us of submission).  -> (uint8 tensor, pinned when a GPU is there, layout)."""
        import numpy as np
        parts = (np.ascontiguousarray(offsets, dtype=np.int64), np.ascontiguousarray(centers, dtype=np.float32),
                 np.ascontiguousarray(labels, dtype=np.int8))
        starts, at = [], 0
        for x in parts:
            starts.append(at)
            at = (at + x.nbytes + 15) & ~15
        blob = torch.empty(max(at, 16), dtype=torch.uint8)
        if pin and torch.cuda.is_available():
            blob = blob.pin_memory()
        for x, st in zip(parts, starts):
            blob[st:st + x.nbytes] = torch.from_numpy(x.reshape(-1).view(np.uint8))
        layout = {"offsets": (starts[0], parts[0].shape[0]), "centers": (starts[1], parts[1].shape[0]),
                  "labels": (starts[2], parts[2].shape[0])}
        return blob, layout

    @staticmethod
    def ragged_views(blob, layout):
        """(centers f32 [S,3], labels i8 [S], offsets i64 [G+1]) as views of a blob of ragged_blob - on whatever device
        the blob lives (the arguments of embed_ragged)."""
        o0, on = layout["offsets"]
        c0, cn = layout["centers"]
        l0, ln = layout["labels"]
        return (blob[c0:c0 + cn * 12].view(torch.float32).view(cn, 3), blob[l0:l0 + ln].view(torch.int8),
                blob[o0:o0 + on * 8].view(torch.int64))

    def ragged_order(self, offsets, node_num, k):
        """size_order for a ragged store: (largest-first launch order i32 device tensor, node_cap).  A graph of c nodes
        in node_num slots has m = node_num - c padding slots, of which one is processed when m >= k (else all m)."""
        if node_num <= MAX_NODES and not self.any_shape and len(offsets) > 1:
            order, info = self.size_order_device(None, None, self._dev(offsets, torch.int64, "offsets"), node_num, k)
            return order, int(info[0].item())
        off = torch.as_tensor(offsets).to(torch.int64).cpu()
        cnt = off[1:] - off[:-1]
        m = node_num - cnt
        eff = cnt + torch.where((m >= k) & (m > 1), torch.ones_like(m), m)
        if eff.numel() == 0:
            return torch.empty(0, dtype=torch.int32, device=self.device), 0
        order = torch.argsort(eff, descending=True, stable=True).to(torch.int32).to(self.device)
        return order, int(eff.max().item())

    def embed_ragged(self, centers, labels, offsets, node_num, k, want_att=False, want_emb=False, node_cap=0, order=None):
        """Ragged store (to_ragged) -> pooled [G,32] (+ att [G,node_num], emb [G,node_num,32]); bit-identical to `embed`
        on the padded arrays.  node_cap / order: see ragged_order."""
        centers = self._dev(centers, torch.float32, "centers")
        labels = self._dev(labels, torch.int8, "labels")
        offsets = self._dev(offsets, torch.int64, "offsets")
        g, n = offsets.numel() - 1, int(node_num)
        assert centers.dim() == 2 and centers.shape[1] == 3 and labels.shape[0] == centers.shape[0], "centers [S,3], labels [S]"
        pooled = torch.empty(g, self.pw, dtype=torch.float32, device=self.device)
        att = torch.empty(g, n, dtype=torch.float32, device=self.device) if want_att else None
        emb = torch.empty(g, n, self.pw, dtype=torch.float32, device=self.device) if want_emb else None
        if g == 0:
            return pooled, att, emb
        ws_bytes = self.lib.sgpr_embed_workspace_bytes(self._h, g, n, k)
        ws = self._ws(ws_bytes)
        if order is not None:
            order = self._dev(order, torch.int32, "order")
        rc = self.lib.sgpr_embed_ragged(self._h, _ptr(centers), _ptr(labels), _ptr(offsets), g, n, int(node_cap), k,
                                        _ptr(order), order.numel() if order is not None else 0, _ptr(pooled), _ptr(att),
                                        _ptr(emb), _ptr(ws), ws_bytes, self._stream())
        self._check(rc)
        return pooled, att, self._cut(emb)

    def embed_dense(self, features, k, want_att=False, want_emb=False):
        """features [G, 3+L, N] f32 (the reference's dense layout) -> pooled (+ att, emb)."""
        features = self._dev(features, torch.float32, "features")
        g, ch, n = features.shape
        if ch != 3 + self.dims.num_labels:
            raise ValueError("features must be [G, %d, N], got %s" % (3 + self.dims.num_labels, tuple(features.shape)))
        pooled = torch.empty(g, self.pw, dtype=torch.float32, device=self.device)
        att = torch.empty(g, n, dtype=torch.float32, device=self.device) if want_att else None
        emb = torch.empty(g, n, self.pw, dtype=torch.float32, device=self.device) if want_emb else None
        ws_bytes = self.lib.sgpr_embed_workspace_bytes(self._h, g, n, k)
        ws = self._ws(ws_bytes)
        rc = self.lib.sgpr_embed_dense(self._h, _ptr(features), g, n, k, _ptr(pooled), _ptr(att), _ptr(emb), _ptr(ws),
                                       ws_bytes, self._stream())
        self._check(rc)
        return pooled, att, self._cut(emb)

    # ------------------------------------------------------------------ pair-coupled half
    def score_pairs(self, pooled1, pooled2, idx1=None, idx2=None, out=None):
        pooled1 = self._pooled(pooled1, "pooled1")
        pooled2 = self._pooled(pooled2, "pooled2")
        if idx1 is not None:
            idx1 = self._dev(idx1, torch.int32, "idx1")
        if idx2 is not None:
            idx2 = self._dev(idx2, torch.int32, "idx2")
        n = idx1.numel() if idx1 is not None else pooled1.shape[0]
        n2 = idx2.numel() if idx2 is not None else pooled2.shape[0]
        if n != n2:
            raise ValueError("pair sides differ in length: %d vs %d" % (n, n2))
        score = out if out is not None else torch.empty(n, dtype=torch.float32, device=self.device)
        rc = self.lib.sgpr_score_pairs(self._h, _ptr(pooled1), _ptr(idx1), _ptr(pooled2), _ptr(idx2), n, _ptr(score),
                                       self._stream())
        self._check(rc)
        return score

    def pair_plan(self, idx1, idx2, num_rows, num_cols):
        """Group a pair list by row graph for score_pair_list (sgpr_pair_plan; host work, once per list - like a launch
        order).  idx1 / idx2: integer arrays on the host (pair p = (idx1[p], idx2[p])).  Returns a PairPlan."""
        return PairPlan(self, idx1, idx2, num_rows, num_cols)

    def score_pair_list(self, pooled_rows, pooled_cols, plan, out=None):
        """score[p] = SG-tail(pooled_rows[idx1[p]], pooled_cols[idx2[p]]) for the pairs of `plan` (sgpr_score_pair_list):
        the bilinear form hoisted per distinct row graph, a row's listed columns through the matrix cores 16 at a time;
        on an f16 handle bit-identical to score_all_pairs' entries at the listed indices (a handle whose tail runs at fp32's
        range - weights or scoring head outside the f16 range, debug bit 13 - scores the list in exact fp32: score_pairs'
        values to rounding)."""
        rows = self._pooled(pooled_rows, "pooled_rows")
        cols = self._pooled(pooled_cols, "pooled_cols")
        if rows.shape[0] != plan.num_rows or cols.shape[0] != plan.num_cols:
            raise ValueError("plan was built for %d x %d graphs, got %d x %d"
                             % (plan.num_rows, plan.num_cols, rows.shape[0], cols.shape[0]))
        score = out if out is not None else torch.empty(plan.P, dtype=torch.float32, device=self.device)
        assert score.numel() == plan.P and score.is_contiguous()
        if plan.P == 0:
            return score
        ws_bytes = self.lib.sgpr_score_pair_list_workspace_bytes(self._h, plan.n_rows, plan.num_cols)
        ws = self._ws(ws_bytes)
        rc = self.lib.sgpr_score_pair_list(self._h, _ptr(rows), plan.num_rows, _ptr(cols), plan.num_cols, _ptr(plan.words),
                                           plan.n_rows, plan.n_items, plan.P, _ptr(score), _ptr(ws), ws_bytes,
                                           self._stream())
        self._check(rc)
        return score

    def score_all_pairs(self, pooled_rows, pooled_cols, out=None):
        rows = self._pooled(pooled_rows, "pooled_rows")
        cols = self._pooled(pooled_cols, "pooled_cols")
        r, m = rows.shape[0], cols.shape[0]
        score = out if out is not None else torch.empty(r, m, dtype=torch.float32, device=self.device)
        assert score.shape == (r, m) and score.stride(1) == 1
        ws_bytes = self.lib.sgpr_score_all_pairs_workspace_bytes(self._h, r, m)
        ws = self._ws(ws_bytes)
        rc = self.lib.sgpr_score_all_pairs(self._h, _ptr(rows), r, _ptr(cols), m, _ptr(score), score.stride(0),
                                           _ptr(ws), ws_bytes, self._stream())
        self._check(rc)
        return score

    MAX_PAIR_JOBS = _C["SGPR_MAX_PAIR_JOBS"]

    def score_all_pairs_multi(self, jobs):
        """Several independent rectangles with one pair of launches (sgpr_score_all_pairs_multi).  jobs: list of
        (pooled_rows, pooled_cols) or (pooled_rows, pooled_cols, out) -> list of [R, M] score tensors."""
        outs, keep, descr = [], [], []
        for job in jobs:
            rows = self._pooled(job[0], "pooled_rows")
            cols = self._pooled(job[1], "pooled_cols")
            out = job[2] if len(job) > 2 and job[2] is not None else torch.empty(rows.shape[0], cols.shape[0],
                                                                                   dtype=torch.float32, device=self.device)
            assert out.shape == (rows.shape[0], cols.shape[0]) and out.stride(1) == 1
            keep.append((rows, cols))
            outs.append(out)
            descr.append(SgprPairsJob(rows.data_ptr(), rows.shape[0], cols.data_ptr(), cols.shape[0], out.data_ptr(),
                                      out.stride(0) if out.shape[0] > 1 else max(out.shape[1], 1)))
        for i in range(0, len(descr), self.MAX_PAIR_JOBS):
            part = descr[i:i + self.MAX_PAIR_JOBS]
            arr = (SgprPairsJob * len(part))(*part)
            ws_bytes = self.lib.sgpr_score_all_pairs_multi_workspace_bytes(self._h, len(part), arr)
            ws = self._ws(ws_bytes)
            rc = self.lib.sgpr_score_all_pairs_multi(self._h, len(part), arr, _ptr(ws), ws_bytes, self._stream())
            self._check(rc)
        return outs

    # ------------------------------------------------------------------ consumers of the score matrix
    def _matrix(self, score, name="score", rank2=False):
        """A resident-matrix argument -> (tensor, R, M, ld).  A float32 2-D tensor on this device with unit column stride
        and a row stride >= M (any strides where there is at most one row / column to step over) is read in place;
        anything else - a host array, another dtype or device, a column-strided or transposed view - is converted once.
        rank2: refuse anything but two dimensions with a ValueError before converting."""
        if not isinstance(score, torch.Tensor):
            score = torch.as_tensor(score)
        if rank2 and score.dim() != 2:
            raise ValueError("%s must be [R, M], got %s" % (name, tuple(score.shape),))
        if not (score.device == self.device and score.dtype == torch.float32 and score.dim() == 2
                and (score.shape[1] <= 1 or score.stride(1) == 1)
                and (score.shape[0] <= 1 or score.stride(0) >= score.shape[1])):
            score = score.to(device=self.device, dtype=torch.float32).contiguous()
        r, m = score.shape
        return score, r, m, max(score.stride(0), m) if r > 1 else m

    def _truth(self, r, m, row0, pose_xz, gt, context=0):
        """the ground truth of the pair consumers -> (pose_xz f64 [>= max(M, row0 + R), 2], None) or, without poses,
        (None, gt i8 [R - context, M]) on the device"""
        if pose_xz is not None:
            pose_xz = self._dev(pose_xz, torch.float64, "pose_xz")
            assert pose_xz.dim() == 2 and pose_xz.shape[1] == 2 and pose_xz.shape[0] >= max(m, row0 + r)
            return pose_xz, None
        if gt is not None:
            gt = self._dev(gt, torch.int8, "gt")
            assert gt.shape == (max(r - int(context), 0), m)
            return None, gt
        raise ValueError("the pair consumers need poses or explicit labels")

    def _positives(self, fn, head, cap, tail=()):
        """a positives list fn(*head, out, capacity, count, *tail, stream): one launch when the list fits the first guess
        (positives are rare: loop closures), a second one sized exactly otherwise -> (scores f32 [n], skipped)"""
        count = torch.empty(2, dtype=torch.int64, device=self.device)
        while True:
            out = torch.empty(cap, dtype=torch.float32, device=self.device)
            self._check(fn(*head, _ptr(out) if cap else None, cap, _ptr(count), *tail, self._stream()))
            n, bad = (int(v) for v in count.tolist())
            if n <= cap:
                return out[:n], bad
            cap = n

    def _threshold_counts(self, fn, head, thresholds, rank, workspace_bytes):
        """a counting pass fn(*head, thresholds, T, rank table, groups per threshold, at_least, out, workspace,
        workspace_bytes, stream), its workspace sized by workspace_bytes(T) -> (counts int64 [T+1], skipped, rank_sum or
        None).  rank = (values, step, above) becomes the sgpr_rank_group table and at_least on the device."""
        thr = self._dev(torch.as_tensor(np.ascontiguousarray(thresholds, dtype=np.float32)), torch.float32, "thresholds")
        t = int(thr.numel())
        out = torch.empty(t + 3, dtype=torch.int64, device=self.device)
        ws_bytes = workspace_bytes(t)
        ws = self._ws(ws_bytes)
        table, at_least, gpt = None, None, 0
        if rank is not None:
            vals, step, above = rank
            vals = np.asarray(vals, dtype=np.float32)
            above = np.asarray(above, dtype=np.int64)
            u, step = int(vals.size), int(step)
            assert above.size == u + 1 and t == -(-u // step) and int(above[0]) < 2 ** 32
            gpt = -(-step // 8)
            # values / pair counts of threshold q's bucket = entries q * step .. (q + 1) * step, padded to gpt * 8
            pad = t * step - u
            v2 = np.concatenate((vals, np.full(pad, np.inf, dtype=np.float32))).reshape(t, step)
            m2 = np.concatenate((above[:-1] - above[1:], np.zeros(pad, dtype=np.int64))).reshape(t, step)
            v3 = np.full((t, gpt * 8), np.inf, dtype=np.float32)
            m3 = np.zeros((t, gpt * 8), dtype=np.uint32)
            v3[:, :step] = v2
            m3[:, :step] = m2
            ent = np.zeros((t, gpt), dtype=RANK_GROUP)
            ent["value"] = v3.reshape(t, gpt, 8)
            ent["pairs"] = m3.reshape(t, gpt, 8)
            table = torch.from_numpy(ent.view(np.uint8).reshape(-1)).to(self.device)
            at_least = torch.from_numpy(np.ascontiguousarray(above[:-1][::step])).to(self.device)
        self._check(fn(*head, _ptr(thr), t, _ptr(table), gpt, _ptr(at_least), _ptr(out), _ptr(ws), ws_bytes,
                       self._stream()))
        h = out.cpu().numpy()
        rank_sum = int(h[t + 2].astype(np.uint64)) if rank is not None else None
        return h[:t + 1].copy(), int(h[t + 1]), rank_sum

    def pair_positives(self, score, row0=0, pose_xz=None, d_pos=3.0, d_neg=20.0, gt=None):
        """Scores of the positive pairs of a rectangle that stays on the device (sgpr_pair_positives): float32 device
        tensor (unordered) and the number of positives skipped for a negative / NaN score."""
        score, r, m, ld = self._matrix(score)
        pose_xz, gt = self._truth(r, m, row0, pose_xz, gt)
        return self._positives(self.lib.sgpr_pair_positives,
                               (self._h, _ptr(score), r, m, ld, int(row0), _ptr(pose_xz), float(d_pos), float(d_neg),
                                _ptr(gt), m), min(r * m, 1 << 20))

    def pair_threshold_counts(self, score, thresholds, row0=0, pose_xz=None, d_pos=3.0, d_neg=20.0, gt=None, rank=None):
        """One streaming pass over a score rectangle (sgpr_pair_threshold_counts): negatives by threshold bucket.
        thresholds: ascending float32 (<= 8191).  rank = (values, step, above) additionally ranks every negative among
        all distinct positive values (see include/sgpr.h).  Returns (counts int64 [T+1], skipped, rank_sum or None)."""
        score, r, m, ld = self._matrix(score)
        pose_xz, gt = self._truth(r, m, row0, pose_xz, gt)
        return self._threshold_counts(self.lib.sgpr_pair_threshold_counts,
                                      (self._h, _ptr(score), r, m, ld, int(row0), _ptr(pose_xz), float(d_pos),
                                       float(d_neg), _ptr(gt), m), thresholds, rank,
                                      lambda t: self.lib.sgpr_pair_threshold_counts_workspace_bytes(self._h, t))

    # ------------------------------------------------------------------ the same consumers without the matrix
    MAX_POOLED_THRESHOLDS = _C["SGPR_SCORE_COUNT_MAX_THRESHOLDS"]

    def score_positives_workspace_bytes(self, r, m):
        return int(self.lib.sgpr_score_positives_workspace_bytes(self._h, int(r), int(m)))

    def score_threshold_counts_workspace_bytes(self, r, m, t):
        return int(self.lib.sgpr_score_threshold_counts_workspace_bytes(self._h, int(r), int(m), int(t)))

    def score_positives(self, pooled_rows, pooled_cols, row0=0, pose_xz=None, d_pos=3.0, d_neg=20.0, gt=None):
        """pair_positives on the rectangle pooled_rows x pooled_cols without forming it (sgpr_score_positives): the
        scores of the positive pairs (float32 device tensor, unordered; bit-identical to score_all_pairs' entries) and
        the number of positives skipped for a negative / NaN score."""
        rows = self._pooled(pooled_rows, "pooled_rows")
        cols = self._pooled(pooled_cols, "pooled_cols")
        r, m = rows.shape[0], cols.shape[0]
        pose_xz, gt = self._truth(r, m, row0, pose_xz, gt)
        ws_bytes = self.score_positives_workspace_bytes(r, m)
        ws = self._ws(ws_bytes)
        return self._positives(self.lib.sgpr_score_positives,
                               (self._h, _ptr(rows), r, _ptr(cols), m, int(row0), _ptr(pose_xz), float(d_pos),
                                float(d_neg), _ptr(gt), m), min(r * m, 1 << 20), (_ptr(ws), ws_bytes))

    def score_threshold_counts(self, pooled_rows, pooled_cols, thresholds, row0=0, pose_xz=None, d_pos=3.0, d_neg=20.0,
                               gt=None, rank=None):
        """pair_threshold_counts on the rectangle pooled_rows x pooled_cols without forming it
        (sgpr_score_threshold_counts): thresholds ascending float32, at most MAX_POOLED_THRESHOLDS.
        Returns (counts int64 [T+1], skipped, rank_sum or None), equal to pair_threshold_counts' on the matrix."""
        rows = self._pooled(pooled_rows, "pooled_rows")
        cols = self._pooled(pooled_cols, "pooled_cols")
        r, m = rows.shape[0], cols.shape[0]
        pose_xz, gt = self._truth(r, m, row0, pose_xz, gt)
        return self._threshold_counts(self.lib.sgpr_score_threshold_counts,
                                      (self._h, _ptr(rows), r, _ptr(cols), m, int(row0), _ptr(pose_xz), float(d_pos),
                                       float(d_neg), _ptr(gt), m), thresholds, rank,
                                      lambda t: self.score_threshold_counts_workspace_bytes(r, m, t))

    def f1_max(self, score, row0=0, pose_xz=None, d_pos=3.0, d_neg=20.0, gt=None):
        """F1-max of a score rectangle in ONE engine call (sgpr_f1_max): every step on the device, one 64-byte copy
        at the end.  Returns the raw result vector (numpy float64 [8], see include/sgpr.h): [0] F1-max, [1] status (0 ok,
        1 = use the multi-call path, 2 = negative / NaN scores), [2] positives, [3] negatives, [4] passes."""
        score, r, m, ld = self._matrix(score)
        pose_xz, gt = self._truth(r, m, row0, pose_xz, gt)
        res = torch.empty(8, dtype=torch.float64, device=self.device)
        ws_bytes = self.lib.sgpr_f1_max_workspace_bytes(self._h, r, m)
        ws = self._ws(ws_bytes)
        rc = self.lib.sgpr_f1_max(self._h, _ptr(score), r, m, ld, int(row0), _ptr(pose_xz), float(d_pos),
                                  float(d_neg), _ptr(gt), m, _ptr(res), _ptr(ws), ws_bytes, self._stream())
        self._check(rc)
        # (the 64 bytes land in a pinned buffer of this engine and thread: a pageable copy is staged by the runtime, and a
        #  buffer shared by the threads of one engine let one thread's copy overwrite another's result before it was read)
        host = getattr(self._host_bufs, "f1", None)
        if host is None:
            host = self._host_bufs.f1 = torch.empty(8, dtype=torch.float64).pin_memory()
        host.copy_(res, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return host.numpy().copy()

    # ------------------------------------------------------------------ ranked lists
    def _row_self(self, row_self, r):
        if row_self is None:
            return None
        rs = self._dev(row_self, torch.int32, "row_self")
        if rs.shape != (r,):
            raise ValueError("row_self must be [%d], got %s" % (r, tuple(rs.shape)))
        return rs

    def _flags(self, causal=False, reverse=_UNSET, positives=_UNSET):
        """The flags word of an entry point and of its *_workspace_bytes twin.  causal: TOPK_CAUSAL.  reverse (the
        sequence family alone passes it): False (forward diagonals c - r = const), True (reverse, c + r = const) or
        "both" (the larger).  positives (the mining calls alone pass it): MINE_POSITIVES or MINE_NEGATIVES."""
        flags = self.TOPK_CAUSAL if causal else 0
        if isinstance(reverse, str):
            if reverse != "both":
                raise ValueError('reverse must be False, True or "both", got %r' % (reverse,))
            flags |= self.SEQ_FORWARD | self.SEQ_REVERSE
        elif reverse is not _UNSET:
            flags |= self.SEQ_REVERSE if reverse else self.SEQ_FORWARD
        if positives is not _UNSET:
            flags |= self.MINE_POSITIVES if positives else self.MINE_NEGATIVES
        return flags

    def _ranked(self, fn, head, ro, k, ws_bytes, codes=False):
        """a ranked-list entry point fn(*head, k, values, indices, [codes,] workspace, workspace_bytes, stream) ->
        (values f32 [ro, k], indices i32 [ro, k]) and, codes, the direction / path codes u8 [ro, k]"""
        outs = [torch.empty(ro, int(k), dtype=dt, device=self.device)
                for dt in (torch.float32, torch.int32, torch.uint8)[:3 if codes else 2]]
        ws = self._ws(ws_bytes)
        self._check(fn(*head, int(k), *[_ptr(t) for t in outs], _ptr(ws), ws_bytes, self._stream()))
        return tuple(outs)

    def topk_rows(self, score, k=1, row0=0, window=-1, causal=False, row_self=None):
        """Best k columns per row outside |col - (row0 + row)| <= window -> (values f32 [R,k], indices i32 [R,k]).
        k in {1, 4, 8, 16} without causal / row_self: sgpr_topk_rows; any other k in 1..4096 (or the causal rule, or a
        row_self table, as score_topk takes them): topk_rows_large."""
        if int(k) in (1, 4, 8, 16) and not causal and row_self is None:
            score, r, m, ld = self._matrix(score)
            vals = torch.empty(r, k, dtype=torch.float32, device=self.device)
            idx = torch.empty(r, k, dtype=torch.int32, device=self.device)
            rc = self.lib.sgpr_topk_rows(self._h, _ptr(score), r, m, ld, int(row0), int(window), int(k),
                                         _ptr(vals), _ptr(idx), self._stream())
            self._check(rc)
            return vals, idx
        return self.topk_rows_large(score, k=k, row0=row0, window=window, causal=causal, row_self=row_self)

    def topk_rows_large_workspace_bytes(self, r, m, k, causal=False):
        return int(self.lib.sgpr_topk_rows_large_workspace_bytes(self._h, int(r), int(m), int(k), self._flags(causal)))

    def topk_rows_large(self, score, k=1, row0=0, window=-1, causal=False, row_self=None):
        """sgpr_topk_rows_large: the best k (1..4096) eligible columns per row of a resident matrix (score_topk's rules:
        window, causal, row_self) -> (values f32 [R,k], indices i32 [R,k]); (-inf, -1) past the last eligible column."""
        score, r, m, ld = self._matrix(score)
        rs = self._row_self(row_self, r)
        flags = self._flags(causal)
        ws_bytes = self.lib.sgpr_topk_rows_large_workspace_bytes(self._h, r, m, int(k), flags)
        return self._ranked(self.lib.sgpr_topk_rows_large,
                            (self._h, _ptr(score), r, m, ld, _ptr(rs), int(row0), int(window), flags), r, k, ws_bytes)

    TOPK_CAUSAL = _C["SGPR_TOPK_CAUSAL"]
    TOPK_LARGE_MAX = _C["SGPR_TOPK_LARGE_MAX"]

    def score_topk_large_workspace_bytes(self, r, m, k, causal=False):
        return int(self.lib.sgpr_score_topk_large_workspace_bytes(self._h, int(r), int(m), int(k), self._flags(causal)))

    def score_topk_large(self, pooled_rows, pooled_cols, k=1, window=-1, row0=0, causal=False, row_self=None):
        """sgpr_score_topk_large: score_topk's lists for k in 1..4096, the rectangle scored in row blocks of at most
        64 MB and each selected as it is written (the large-k selection, whatever k)."""
        rows = self._pooled(pooled_rows, "pooled_rows")
        cols = self._pooled(pooled_cols, "pooled_cols")
        r, m = rows.shape[0], cols.shape[0]
        rs = self._row_self(row_self, r)
        flags = self._flags(causal)
        ws_bytes = self.lib.sgpr_score_topk_large_workspace_bytes(self._h, r, m, int(k), flags)
        return self._ranked(self.lib.sgpr_score_topk_large,
                            (self._h, _ptr(rows), r, _ptr(cols), m, _ptr(rs), int(row0), int(window), flags), r, k,
                            ws_bytes)

    SEQ_FORWARD = _C["SGPR_SEQ_FORWARD"]
    SEQ_REVERSE = _C["SGPR_SEQ_REVERSE"]
    SEQ_MAX_LEN = _C["SGPR_SEQ_MAX_LEN"]

    def _filter_outputs(self, ro, m, out, second=None, second_name=None, want_second=False):
        """The outputs of a filter -> (out f32 [ro, m], second u8 [ro, m] or None, their common row stride).  Given
        tensors are checked - this device, dtype, shape, unit column stride, one row stride >= m shared by both - and
        missing ones allocated (the second one only when wanted)."""
        if out is None:
            out = torch.empty(ro, m, dtype=torch.float32, device=self.device)
        if second is None and want_second:
            second = torch.empty(ro, m, dtype=torch.uint8, device=self.device)
        ldo = m
        for t, dt, name in ((out, torch.float32, "out"), (second, torch.uint8, second_name)):
            if t is None:
                continue
            if (t.device != self.device or t.dtype != dt or tuple(t.shape) != (ro, m) or (m > 1 and t.stride(1) != 1)
                    or (ro > 1 and t.stride(0) < m)):
                raise ValueError("%s must be a %s device tensor [%d, %d] with unit column stride" % (name, dt, ro, m))
            if ro > 1:
                ldo = max(ldo, t.stride(0))
        if ro > 1 and second is not None and out.stride(0) != second.stride(0):
            raise ValueError("out and %s must share one row stride" % second_name)
        return out, second, ldo

    def seq_filter(self, score, seq_len, context=0, reverse=False, want_dir=False, out=None, out_dir=None):
        """sgpr_seq_filter: the mean of a resident matrix along the diagonal of up to seq_len entries that ends in
        (r, c) - rows and columns in trajectory order - for rows context .. R-1 -> Q f32 [R - context, M] (and, want_dir,
        the direction taken, u8: 0 forward, 1 reverse).  fp32 sums in a fixed order: bit-reproducible (include/sgpr.h).
        A row-strided view (unit column stride) is read in place.  out / out_dir: device tensors [R - context, M] to
        write into, with one common row stride >= M and unit column stride (they must not overlap score)."""
        score, r, m, ld = self._matrix(score, rank2=True)
        out, out_dir, ldo = self._filter_outputs(max(r - int(context), 0), m, out, out_dir, "out_dir", want_dir)
        rc = self.lib.sgpr_seq_filter(self._h, _ptr(score), r, m, ld, int(context), int(seq_len),
                                      self._flags(reverse=reverse), _ptr(out), ldo, _ptr(out_dir), self._stream())
        self._check(rc)
        return out if out_dir is None else (out, out_dir)

    def score_seq_topk_workspace_bytes(self, r, m, seq_len, k=1, causal=False, context=0, reverse="both"):
        return int(self.lib.sgpr_score_seq_topk_workspace_bytes(self._h, int(r), int(m), int(context), int(seq_len),
                                                                int(k), self._flags(causal, reverse)))

    def score_seq_topk(self, pooled_rows, pooled_cols, seq_len, k=1, window=-1, row0=0, causal=False, row_self=None,
                       context=0, reverse="both"):
        """sgpr_score_seq_topk: score_topk_large's lists of the sequence-matched score (seq_filter of the rectangle,
        never formed beyond 64 MB row blocks) for rows context .. R-1 -> (values f32 [R - context, k], indices i32,
        dirs u8: 0 forward, 1 reverse, 0 in a padding slot).  Eligibility is score_topk's on the end point, with
        row_self [R] / row0 + r counted over all R rows."""
        rows = self._pooled(pooled_rows, "pooled_rows")
        cols = self._pooled(pooled_cols, "pooled_cols")
        r, m = rows.shape[0], cols.shape[0]
        rs = self._row_self(row_self, r)
        flags = self._flags(causal, reverse)
        ws_bytes = self.lib.sgpr_score_seq_topk_workspace_bytes(self._h, r, m, int(context), int(seq_len), int(k), flags)
        return self._ranked(self.lib.sgpr_score_seq_topk,
                            (self._h, _ptr(rows), r, _ptr(cols), m, int(context), _ptr(rs), int(row0), int(window), flags,
                             int(seq_len)), max(r - int(context), 0), k, ws_bytes, codes=True)

    SEQ_MAX_PATHS = SEQ_MAX_PATHS
    SEQ_PATH_MAX_OFFSET = SEQ_PATH_MAX_OFFSET

    def seq_path_filter(self, score, seq_len, paths, context=0, reverse=False, want_code=False, out=None, out_code=None):
        """sgpr_seq_path_filter: seq_filter maximised over a set of paths (int32 [P, seq_len], see seq_paths) -> Q f32
        [R - context, M] (and, want_code, the winner's code u8: direction bit | path << 1).  The single path
        off[d] = d gives seq_filter's bits.  out / out_code as seq_filter's out / out_dir."""
        score, r, m, ld = self._matrix(score, rank2=True)
        table = _path_table(paths, seq_len)
        out, out_code, ldo = self._filter_outputs(max(r - int(context), 0), m, out, out_code, "out_code", want_code)
        rc = self.lib.sgpr_seq_path_filter(self._h, _ptr(score), r, m, ld, int(context), int(seq_len),
                                           self._flags(reverse=reverse), *_table_args(table), _ptr(out),
                                           ldo, _ptr(out_code), self._stream())
        self._check(rc)
        return out if out_code is None else (out, out_code)

    def score_path_topk_workspace_bytes(self, r, m, seq_len, n_paths, k=1, radius=0, causal=False, context=0,
                                        reverse="both"):
        return int(self.lib.sgpr_score_path_topk_workspace_bytes(self._h, int(r), int(m), int(context), int(seq_len),
                                                                 int(n_paths), int(k), int(radius),
                                                                 self._flags(causal, reverse)))

    def score_path_topk(self, pooled_rows, pooled_cols, seq_len, paths, k=1, radius=0, window=-1, row0=0, causal=False,
                        row_self=None, context=0, reverse="both"):
        """sgpr_score_path_topk: score_seq_topk's (radius 0) or score_peak_topk's (radius > 0) lists of the path-set
        score (seq_path_filter of the rectangle, never formed beyond 64 MB row blocks) for rows context .. R-1 ->
        (values f32 [R - context, k], indices i32, codes u8: direction bit | path << 1, 0 in a padding slot)."""
        rows = self._pooled(pooled_rows, "pooled_rows")
        cols = self._pooled(pooled_cols, "pooled_cols")
        table = _path_table(paths, seq_len)
        r, m = rows.shape[0], cols.shape[0]
        rs = self._row_self(row_self, r)
        flags = self._flags(causal, reverse)
        ws_bytes = self.lib.sgpr_score_path_topk_workspace_bytes(self._h, r, m, int(context), int(seq_len),
                                                                 table.shape[0], int(k), int(radius), flags)
        return self._ranked(self.lib.sgpr_score_path_topk,
                            (self._h, _ptr(rows), r, _ptr(cols), m, int(context), _ptr(rs), int(row0), int(window), flags,
                             int(seq_len), *_table_args(table), int(radius)),
                            max(r - int(context), 0), k, ws_bytes, codes=True)

    SESSION_MAX = SESSION_MAX

    @staticmethod
    def _session_tables(paths, seq_len, row_sessions, col_sessions):
        """(path table pointer, n_paths, row table pointer, n, column table pointer, n) and the arrays that own them"""
        table = None if paths is None else _path_table(paths, seq_len)
        rt, ct = _session_table(row_sessions), _session_table(col_sessions)
        return [*_table_args(table), *_table_args(rt), *_table_args(ct)], (table, rt, ct)

    def session_filter(self, score, seq_len, paths=None, row_sessions=None, col_sessions=None, window=-1, row0=0,
                       row_self=None, context=0, reverse=False, want_code=False, out=None, out_code=None):
        """sgpr_session_filter: seq_path_filter on a stacked multi-session matrix.  row_sessions / col_sessions: the
        first row / column of every session (int32, starting at 0, non-decreasing; None: one session).  Sums stop at the
        edges of the end point's own row and column session; with window >= 0 column c is excluded (-inf, code 0) for
        row r iff it lies in the session of self_r (row_self[r] or row0 + r) and |c - self_r| <= window.  paths None: the
        unit diagonal.  -> Q f32 [R - context, M] (and, want_code, the code u8).  out / out_code as seq_filter's."""
        score, r, m, ld = self._matrix(score, rank2=True)
        tables, keep = self._session_tables(paths, seq_len, row_sessions, col_sessions)
        rs = self._row_self(row_self, r)
        out, out_code, ldo = self._filter_outputs(max(r - int(context), 0), m, out, out_code, "out_code", want_code)
        rc = self.lib.sgpr_session_filter(self._h, _ptr(score), r, m, ld, int(context), int(seq_len),
                                          self._flags(reverse=reverse), *tables, _ptr(rs), int(row0), int(window),
                                          _ptr(out), ldo, _ptr(out_code), self._stream())
        self._check(rc)
        return out if out_code is None else (out, out_code)

    def score_session_topk_workspace_bytes(self, r, m, seq_len, n_paths=0, k=1, causal=False, context=0, reverse="both",
                                           n_row_sessions=0, n_col_sessions=0):
        return int(self.lib.sgpr_score_session_topk_workspace_bytes(self._h, int(r), int(m), int(context), int(seq_len),
                                                                    int(n_paths), int(k), self._flags(causal, reverse),
                                                                    int(n_row_sessions), int(n_col_sessions)))

    def score_session_topk(self, pooled_rows, pooled_cols, seq_len, paths=None, row_sessions=None, col_sessions=None, k=1,
                           window=-1, row0=0, causal=False, row_self=None, context=0, reverse="both"):
        """sgpr_score_session_topk: score_path_topk's lists (radius 0) of the session-aware score (session_filter of
        the rectangle, never formed beyond 64 MB row blocks) for rows context .. R-1 -> (values f32 [R - context, k],
        indices i32, codes u8).  row_sessions counts over all R rows, the context rows included."""
        rows = self._pooled(pooled_rows, "pooled_rows")
        cols = self._pooled(pooled_cols, "pooled_cols")
        tables, keep = self._session_tables(paths, seq_len, row_sessions, col_sessions)
        r, m = rows.shape[0], cols.shape[0]
        rs = self._row_self(row_self, r)
        flags = self._flags(causal, reverse)
        ws_bytes = self.lib.sgpr_score_session_topk_workspace_bytes(self._h, r, m, int(context), int(seq_len), tables[1],
                                                                    int(k), flags, tables[3], tables[5])
        return self._ranked(self.lib.sgpr_score_session_topk,
                            (self._h, _ptr(rows), r, _ptr(cols), m, int(context), _ptr(rs), int(row0), int(window), flags,
                             int(seq_len), *tables), max(r - int(context), 0), k, ws_bytes, codes=True)

    PEAK_MAX_RADIUS = _C["SGPR_PEAK_MAX_RADIUS"]
    PEAK_STRIP = _C["SGPR_PEAK_STRIP"]           # columns a workgroup of the peak filter owns

    def peak_filter(self, score, radius, window=-1, row0=0, causal=False, row_self=None, out=None):
        """sgpr_peak_filter: a resident matrix [R, M] -> P f32 [R, M]: the score at a PEAK - a qualifying column
        (score_topk's eligibility: window, causal, row_self / row0; neither NaN nor -inf) that comes first, by (value
        descending, column ascending), among the qualifying columns at most `radius` away - and -inf elsewhere.
        A row-strided view (unit column stride) is read in place.  out: a device tensor [R, M] to write into (row
        stride >= M, unit column stride; it must not overlap score)."""
        score, r, m, ld = self._matrix(score, rank2=True)
        rs = self._row_self(row_self, r)
        out, _, ldo = self._filter_outputs(r, m, out)
        rc = self.lib.sgpr_peak_filter(self._h, _ptr(score), r, m, ld, _ptr(rs), int(row0), int(window),
                                       self._flags(causal), int(radius), _ptr(out), ldo, self._stream())
        self._check(rc)
        return out

    def score_peak_topk_workspace_bytes(self, r, m, radius, seq_len=1, k=1, causal=False, context=0, reverse=False):
        return int(self.lib.sgpr_score_peak_topk_workspace_bytes(self._h, int(r), int(m), int(context), int(seq_len),
                                                                 int(k), int(radius), self._flags(causal, reverse)))

    def score_peak_topk(self, pooled_rows, pooled_cols, radius, seq_len=1, k=1, window=-1, row0=0, causal=False,
                        row_self=None, context=0, reverse=False):
        """sgpr_score_peak_topk: distinct-place loop closures - the k best peaks (peak_filter's definition, within
        `radius` columns) of the sequence-matched score (seq_len = 1: of the score itself) for rows context .. R-1 ->
        (values f32 [R - context, k], indices i32, dirs u8), (-inf, -1, 0) past the last peak.  score_seq_topk's
        arguments and rules; radius = 0 returns its bits.  Choose radius <= window: the first eligible column beside
        an excluded window can be a peak of a slope that rises into the window."""
        rows = self._pooled(pooled_rows, "pooled_rows")
        cols = self._pooled(pooled_cols, "pooled_cols")
        r, m = rows.shape[0], cols.shape[0]
        rs = self._row_self(row_self, r)
        flags = self._flags(causal, reverse)
        ws_bytes = self.lib.sgpr_score_peak_topk_workspace_bytes(self._h, r, m, int(context), int(seq_len), int(k),
                                                                 int(radius), flags)
        return self._ranked(self.lib.sgpr_score_peak_topk,
                            (self._h, _ptr(rows), r, _ptr(cols), m, int(context), _ptr(rs), int(row0), int(window), flags,
                             int(seq_len), int(radius)), max(r - int(context), 0), k, ws_bytes, codes=True)

    def score_topk_workspace_bytes(self, r, m, k=1, causal=False):
        return int(self.lib.sgpr_score_topk_workspace_bytes(self._h, int(r), int(m), int(k), self._flags(causal)))

    def score_topk(self, pooled_rows, pooled_cols, k=1, window=-1, row0=0, causal=False, row_self=None):
        """Best k columns per row of the rectangle pooled_rows x pooled_cols without forming it (sgpr_score_topk):
        column c qualifies for row r iff |c - self_r| > window (window < 0: no window) and, causal, c < self_r, where
        self_r = row_self[r] or row0 + r.  -> (values f32 [R,k], indices i32 [R,k]); every value is bit-identical to
        score_all_pairs' entry (r, c); (-inf, -1) where fewer than k columns qualify.  k in 17..4096: score_topk_large."""
        if int(k) > 16:
            return self.score_topk_large(pooled_rows, pooled_cols, k=k, window=window, row0=row0, causal=causal,
                                         row_self=row_self)
        rows = self._pooled(pooled_rows, "pooled_rows")
        cols = self._pooled(pooled_cols, "pooled_cols")
        r, m = rows.shape[0], cols.shape[0]
        rs = self._row_self(row_self, r)
        flags = self._flags(causal)
        ws_bytes = self.lib.sgpr_score_topk_workspace_bytes(self._h, r, m, int(k), flags)
        return self._ranked(self.lib.sgpr_score_topk,
                            (self._h, _ptr(rows), r, _ptr(cols), m, _ptr(rs), int(row0), int(window), flags), r, k,
                            ws_bytes)

    MINE_NEGATIVES = _C["SGPR_MINE_NEGATIVES"]
    MINE_POSITIVES = _C["SGPR_MINE_POSITIVES"]

    def _mine_poses(self, col_pose, row_pose, r, m):
        """[.,12] KITTI or [.,2] planar poses -> float64 (x, z) device tensors ([m,2] columns, [r,2] rows or None)"""
        def planar(p, n, name):
            p = torch.as_tensor(p) if not isinstance(p, torch.Tensor) else p
            if p.dim() != 2 or p.shape[1] not in (2, 12) or p.shape[0] != n:
                raise ValueError("%s must be [%d, 12] (KITTI 3x4) or [%d, 2] planar (x, z), got %s"
                                 % (name, n, n, tuple(p.shape)))
            if p.shape[1] == 12:
                p = p[:, [3, 11]]
            return self._dev(p, torch.float64, name)
        return planar(col_pose, m, "col_pose"), None if row_pose is None else planar(row_pose, r, "row_pose")

    def score_mine_workspace_bytes(self, r, m, k=1, positives=False, causal=False):
        return int(self.lib.sgpr_score_mine_workspace_bytes(self._h, int(r), int(m), int(k),
                                                            self._flags(causal, positives=positives)))

    def score_mine(self, pooled_rows, pooled_cols, col_pose, k=1, positives=False, d_pos=3.0, d_neg=20.0, window=-1,
                   row0=0, causal=False, row_self=None, row_pose=None):
        """The k hardest pose-labelled pairs per row of pooled_rows x pooled_cols without forming the matrix
        (sgpr_score_mine).  Column c is eligible for row r iff it is for score_topk and c != self_r; the pair's class
        comes from the float64 distance of the row pose (row_pose[r], else col_pose[self_r]) to col_pose[c].
        positives=False: negatives (distance >= d_neg), highest score first; (-inf, -1) in empty slots.
        positives=True: positives (distance <= d_pos), lowest score first; (+inf, -1) in empty slots.
        Poses are [.,12] KITTI or [.,2] planar.  -> (values f32 [R,k], indices i32 [R,k]); every value is
        bit-identical to score_all_pairs' entry (r, c)."""
        rows = self._pooled(pooled_rows, "pooled_rows")
        cols = self._pooled(pooled_cols, "pooled_cols")
        r, m = rows.shape[0], cols.shape[0]
        cp, rp = self._mine_poses(col_pose, row_pose, r, m)
        rs = self._row_self(row_self, r)
        flags = self._flags(causal, positives=positives)
        ws_bytes = self.lib.sgpr_score_mine_workspace_bytes(self._h, r, m, int(k), flags)
        return self._ranked(self.lib.sgpr_score_mine,
                            (self._h, _ptr(rows), r, _ptr(cols), m, _ptr(cp), _ptr(rp), _ptr(rs), int(row0), int(window),
                             flags, float(d_pos), float(d_neg)), r, k, ws_bytes)

    def mine_rows(self, score, col_pose, k=1, positives=False, d_pos=3.0, d_neg=20.0, window=-1, row0=0, causal=False,
                  row_self=None, row_pose=None):
        """score_mine's selection on a resident matrix score [R, M] (sgpr_mine_rows; any row stride >= M with unit
        column stride is read in place) -> (values f32 [R,k], indices i32 [R,k])."""
        score, r, m, ld = self._matrix(score)
        cp, rp = self._mine_poses(col_pose, row_pose, r, m)
        rs = self._row_self(row_self, r)
        flags = self._flags(causal, positives=positives)
        ws_bytes = self.lib.sgpr_mine_rows_workspace_bytes(self._h, r, m, int(k), flags)
        return self._ranked(self.lib.sgpr_mine_rows,
                            (self._h, _ptr(score), r, m, ld, _ptr(cp), _ptr(rp), _ptr(rs), int(row0), int(window), flags,
                             float(d_pos), float(d_neg)), r, k, ws_bytes)

    def score_above_workspace_bytes(self, r, m, causal=False):
        return int(self.lib.sgpr_score_above_workspace_bytes(self._h, int(r), int(m), self._flags(causal)))

    def rows_above_workspace_bytes(self, r, m):
        return int(self.lib.sgpr_rows_above_workspace_bytes(self._h, int(r), int(m)))

    @staticmethod
    def above_estimate(r, m):
        """first output capacity of score_above / rows_above with capacity=None"""
        return min(int(r) * int(m), max(1 << 16, 16 * int(r)))

    def _above(self, r, m, capacity, call):
        """run call(cap, rows, cols, values, row_ptr, count) -> rc: with capacity=None once at above_estimate and, if
        the count read back exceeds it, once more at the exact count; else once, asynchronously"""
        def run(cap):
            out_r = torch.empty(cap, dtype=torch.int32, device=self.device)
            out_c = torch.empty(cap, dtype=torch.int32, device=self.device)
            out_v = torch.empty(cap, dtype=torch.float32, device=self.device)
            row_ptr = torch.empty(r + 1, dtype=torch.int64, device=self.device)
            count = torch.empty(1, dtype=torch.int64, device=self.device)
            self._check(call(cap, out_r, out_c, out_v, row_ptr, count))
            return out_r, out_c, out_v, row_ptr, count
        if capacity is not None:
            if int(capacity) < 0:
                raise ValueError("capacity must be >= 0, got %d" % int(capacity))
            return run(int(capacity))[:4]
        cap = self.above_estimate(r, m)
        out_r, out_c, out_v, row_ptr, count = run(cap)
        n = int(count.item())                               # the one synchronisation
        if n > cap:
            out_r, out_c, out_v, row_ptr, count = run(n)
        return out_r[:n], out_c[:n], out_v[:n], row_ptr

    def score_above(self, pooled_rows, pooled_cols, threshold, window=-1, row0=0, causal=False, row_self=None,
                    capacity=None):
        """Every pair (r, c) of the rectangle pooled_rows x pooled_cols with score >= threshold, without forming the
        matrix (sgpr_score_above).  Column c is eligible for row r iff |c - self_r| > window (window < 0: no window)
        and, causal, c < self_r, where self_r = row_self[r] or row0 + r; NaN scores never qualify.
        -> (rows i32 [n], cols i32 [n], values f32 [n], row_ptr i64 [R+1]) on the device, row-major (r, then c
        ascending); every value is bit-identical to score_all_pairs' entry (r, c); row_ptr[-1] is the exact total.
        capacity=None: the call runs at an estimated capacity and reads the 8-byte count back - the only host
        synchronisation -; if more pairs qualify it runs again at the exact count, and n = the total.
        capacity=K: fully asynchronous; the arrays are [K] and hold the first min(total, K) pairs (the rest of them
        is undefined when fewer qualify: row_ptr[-1] tells how many)."""
        if threshold != threshold:
            raise ValueError("threshold is NaN")
        rows = self._pooled(pooled_rows, "pooled_rows")
        cols = self._pooled(pooled_cols, "pooled_cols")
        r, m = rows.shape[0], cols.shape[0]
        rs = self._row_self(row_self, r)
        flags = self._flags(causal)
        ws_bytes = self.lib.sgpr_score_above_workspace_bytes(self._h, r, m, flags)
        ws = self._ws(ws_bytes)

        def call(cap, out_r, out_c, out_v, row_ptr, count):
            return self.lib.sgpr_score_above(self._h, _ptr(rows), r, _ptr(cols), m, _ptr(rs), int(row0), int(window),
                                             flags, float(threshold), _ptr(out_r), _ptr(out_c), _ptr(out_v), cap,
                                             _ptr(row_ptr), _ptr(count), _ptr(ws), ws_bytes, self._stream())
        return self._above(r, m, capacity, call)

    def rows_above(self, score, threshold, window=-1, row0=0, causal=False, row_self=None, capacity=None):
        """score_above's selection on a resident matrix score [R, M] (sgpr_rows_above; any row stride >= M with unit
        column stride is read in place) -> (rows, cols, values, row_ptr), with score_above's rules and capacity."""
        if threshold != threshold:
            raise ValueError("threshold is NaN")
        score, r, m, ld = self._matrix(score)
        rs = self._row_self(row_self, r)
        flags = self._flags(causal)
        ws_bytes = self.lib.sgpr_rows_above_workspace_bytes(self._h, r, m)
        ws = self._ws(ws_bytes)

        def call(cap, out_r, out_c, out_v, row_ptr, count):
            return self.lib.sgpr_rows_above(self._h, _ptr(score), r, m, ld, _ptr(rs), int(row0), int(window), flags,
                                            float(threshold), _ptr(out_r), _ptr(out_c), _ptr(out_v), cap,
                                            _ptr(row_ptr), _ptr(count), _ptr(ws), ws_bytes, self._stream())
        return self._above(r, m, capacity, call)

    # ------------------------------------------------------------------ the same on the sequence-matched score
    def seq_rows_above_workspace_bytes(self, r, m, context=0):
        return int(self.lib.sgpr_seq_rows_above_workspace_bytes(self._h, int(r), int(m), int(context)))

    def score_seq_above_workspace_bytes(self, r, m, seq_len, causal=False, context=0, reverse="both"):
        flags = self._flags(causal, reverse)
        return int(self.lib.sgpr_score_seq_above_workspace_bytes(self._h, int(r), int(m), int(context), int(seq_len),
                                                                 flags))

    def _seq_above(self, r, m, context, capacity, call, want_dirs=True):
        """_above for the outputs of rows context .. r - 1, with the direction of every listed pair"""
        ro = max(r - int(context), 0)
        dirs = []

        def call_dirs(cap, out_r, out_c, out_v, row_ptr, count):
            d = torch.empty(cap, dtype=torch.uint8, device=self.device) if want_dirs else None
            dirs[:] = [d]
            return call(cap, out_r, out_c, out_v, d, row_ptr, count)
        out_r, out_c, out_v, row_ptr = self._above(ro, m, capacity, call_dirs)
        d = dirs[0]
        return out_r, out_c, out_v, (d[:out_r.numel()] if d is not None else None), row_ptr

    def seq_rows_above(self, score, seq_len, threshold, window=-1, row0=0, causal=False, row_self=None, context=0,
                       reverse="both", capacity=None, want_dirs=True):
        """rows_above on the sequence-matched score of a resident matrix score [R, M] (sgpr_seq_rows_above; any row
        stride >= M with unit column stride is read in place): every eligible pair of rows context .. R-1 whose
        seq_filter value is >= threshold -> (rows i32 [n] counted from `context`, cols i32 [n], values f32 [n] - the bits
        seq_filter writes -, dirs u8 [n] (0 forward, 1 reverse; None for want_dirs=False), row_ptr i64 [R - context + 1]),
        row-major.  Eligibility is score_topk's on the end point, with row_self [R] / row0 + r counted over all R rows;
        capacity as in score_above.  The filtered matrix is never written."""
        if threshold != threshold:
            raise ValueError("threshold is NaN")
        score, r, m, ld = self._matrix(score)
        rs = self._row_self(row_self, r)
        flags = self._flags(causal, reverse)
        ws_bytes = self.lib.sgpr_seq_rows_above_workspace_bytes(self._h, r, m, int(context))
        ws = self._ws(ws_bytes)

        def call(cap, out_r, out_c, out_v, out_d, row_ptr, count):
            return self.lib.sgpr_seq_rows_above(self._h, _ptr(score), r, m, ld, int(context), _ptr(rs), int(row0),
                                                int(window), flags, int(seq_len), float(threshold), _ptr(out_r),
                                                _ptr(out_c), _ptr(out_v), _ptr(out_d), cap, _ptr(row_ptr), _ptr(count),
                                                _ptr(ws), ws_bytes, self._stream())
        return self._seq_above(r, m, context, capacity, call, want_dirs)

    def score_seq_above(self, pooled_rows, pooled_cols, seq_len, threshold, window=-1, row0=0, causal=False,
                        row_self=None, context=0, reverse="both", capacity=None, want_dirs=True):
        """seq_rows_above on the rectangle pooled_rows x pooled_cols without forming it (sgpr_score_seq_above): the
        rectangle is scored in row blocks of at most 64 MB that carry their last seq_len - 1 rows over as context, and
        neither the filtered scores nor their directions are ever stored -> (rows, cols, values, dirs, row_ptr)."""
        if threshold != threshold:
            raise ValueError("threshold is NaN")
        rows = self._pooled(pooled_rows, "pooled_rows")
        cols = self._pooled(pooled_cols, "pooled_cols")
        r, m = rows.shape[0], cols.shape[0]
        rs = self._row_self(row_self, r)
        flags = self._flags(causal, reverse)
        ws_bytes = self.lib.sgpr_score_seq_above_workspace_bytes(self._h, r, m, int(context), int(seq_len), flags)
        ws = self._ws(ws_bytes)

        def call(cap, out_r, out_c, out_v, out_d, row_ptr, count):
            return self.lib.sgpr_score_seq_above(self._h, _ptr(rows), r, _ptr(cols), m, int(context), _ptr(rs), int(row0),
                                                 int(window), flags, int(seq_len), float(threshold), _ptr(out_r),
                                                 _ptr(out_c), _ptr(out_v), _ptr(out_d), cap, _ptr(row_ptr), _ptr(count),
                                                 _ptr(ws), ws_bytes, self._stream())
        return self._seq_above(r, m, context, capacity, call, want_dirs)

    # ------------------------------------------------------------------ ... and on the session-aware path-set score
    def session_rows_above_workspace_bytes(self, r, m, context=0):
        return int(self.lib.sgpr_session_rows_above_workspace_bytes(self._h, int(r), int(m), int(context)))

    def score_session_above_workspace_bytes(self, r, m, seq_len, n_paths=0, causal=False, context=0, reverse="both",
                                            n_row_sessions=0, n_col_sessions=0):
        flags = self._flags(causal, reverse)
        return int(self.lib.sgpr_score_session_above_workspace_bytes(self._h, int(r), int(m), int(context), int(seq_len),
                                                                     int(n_paths), flags, int(n_row_sessions),
                                                                     int(n_col_sessions)))

    def session_rows_above(self, score, seq_len, threshold, paths=None, row_sessions=None, col_sessions=None, min_terms=1,
                           window=-1, row0=0, causal=False, row_self=None, context=0, reverse="both", capacity=None,
                           want_codes=True):
        """seq_rows_above on the session-aware path-set score of a resident matrix score [R, M]
        (sgpr_session_rows_above): every eligible pair of rows context .. R-1 whose session_filter value, folded over
        the candidates with at least `min_terms` terms, is >= threshold -> (rows i32 [n] counted from `context`, cols
        i32 [n], values f32 [n], codes u8 [n] (direction bit | path << 1; None for want_codes=False), row_ptr i64
        [R - context + 1]), row-major.  paths / row_sessions / col_sessions / window as session_filter's; an end point
        none of whose candidates has min_terms terms is never listed; capacity as in score_above."""
        if threshold != threshold:
            raise ValueError("threshold is NaN")
        score, r, m, ld = self._matrix(score)
        rs = self._row_self(row_self, r)
        tables, keep = self._session_tables(paths, seq_len, row_sessions, col_sessions)
        flags = self._flags(causal, reverse)
        ws_bytes = self.lib.sgpr_session_rows_above_workspace_bytes(self._h, r, m, int(context))
        ws = self._ws(ws_bytes)

        def call(cap, out_r, out_c, out_v, out_d, row_ptr, count):
            return self.lib.sgpr_session_rows_above(self._h, _ptr(score), r, m, ld, int(context), _ptr(rs), int(row0),
                                                    int(window), flags, int(seq_len), *tables, int(min_terms),
                                                    float(threshold), _ptr(out_r), _ptr(out_c), _ptr(out_v),
                                                    _ptr(out_d), cap, _ptr(row_ptr), _ptr(count), _ptr(ws), ws_bytes,
                                                    self._stream())
        return self._seq_above(r, m, context, capacity, call, want_codes)

    def score_session_above(self, pooled_rows, pooled_cols, seq_len, threshold, paths=None, row_sessions=None,
                            col_sessions=None, min_terms=1, window=-1, row0=0, causal=False, row_self=None, context=0,
                            reverse="both", capacity=None, want_codes=True):
        """session_rows_above on the rectangle pooled_rows x pooled_cols without forming it (sgpr_score_session_above):
        score_seq_above's row blocks with the row table moving with each block; neither the filtered scores nor their
        codes are ever stored -> (rows, cols, values, codes, row_ptr).  row_sessions counts over all R rows, the
        context rows included."""
        if threshold != threshold:
            raise ValueError("threshold is NaN")
        rows = self._pooled(pooled_rows, "pooled_rows")
        cols = self._pooled(pooled_cols, "pooled_cols")
        r, m = rows.shape[0], cols.shape[0]
        rs = self._row_self(row_self, r)
        tables, keep = self._session_tables(paths, seq_len, row_sessions, col_sessions)
        flags = self._flags(causal, reverse)
        ws_bytes = self.lib.sgpr_score_session_above_workspace_bytes(self._h, r, m, int(context), int(seq_len), tables[1],
                                                                     flags, tables[3], tables[5])
        ws = self._ws(ws_bytes)

        def call(cap, out_r, out_c, out_v, out_d, row_ptr, count):
            return self.lib.sgpr_score_session_above(self._h, _ptr(rows), r, _ptr(cols), m, int(context), _ptr(rs),
                                                     int(row0), int(window), flags, int(seq_len), *tables, int(min_terms),
                                                     float(threshold), _ptr(out_r), _ptr(out_c), _ptr(out_v),
                                                     _ptr(out_d), cap, _ptr(row_ptr), _ptr(count), _ptr(ws), ws_bytes,
                                                     self._stream())
        return self._seq_above(r, m, context, capacity, call, want_codes)

    def score_seq_positives_workspace_bytes(self, r, m, seq_len, context=0, reverse="both"):
        return int(self.lib.sgpr_score_seq_positives_workspace_bytes(self._h, int(r), int(m), int(context), int(seq_len),
                                                                     self._flags(reverse=reverse)))

    def score_seq_threshold_counts_workspace_bytes(self, r, m, seq_len, t, context=0, reverse="both"):
        return int(self.lib.sgpr_score_seq_threshold_counts_workspace_bytes(self._h, int(r), int(m), int(context),
                                                                            int(seq_len), self._flags(reverse=reverse), int(t)))

    def score_seq_positives(self, pooled_rows, pooled_cols, seq_len, row0=0, pose_xz=None, d_pos=3.0, d_neg=20.0, gt=None,
                            context=0, reverse="both"):
        """pair_positives on seq_filter(score_all_pairs(pooled_rows, pooled_cols)) without the matrix
        (sgpr_score_seq_positives): the sequence-matched scores of the positive pairs of rows context .. R-1 (float32
        device tensor, unordered, the bits seq_filter writes) and the number skipped for a negative / NaN score.  The row
        pose of output row o is pose_xz[row0 + context + o]; gt is [R - context, M]."""
        rows = self._pooled(pooled_rows, "pooled_rows")
        cols = self._pooled(pooled_cols, "pooled_cols")
        r, m = rows.shape[0], cols.shape[0]
        pose_xz, gt = self._truth(r, m, row0, pose_xz, gt, context)
        flags = self._flags(reverse=reverse)
        ws_bytes = self.lib.sgpr_score_seq_positives_workspace_bytes(self._h, r, m, int(context), int(seq_len), flags)
        ws = self._ws(ws_bytes)
        return self._positives(self.lib.sgpr_score_seq_positives,
                               (self._h, _ptr(rows), r, _ptr(cols), m, int(context), int(seq_len), flags, int(row0),
                                _ptr(pose_xz), float(d_pos), float(d_neg), _ptr(gt), m),
                               min(max(r - int(context), 0) * m, 1 << 20), (_ptr(ws), ws_bytes))

    def score_seq_threshold_counts(self, pooled_rows, pooled_cols, seq_len, thresholds, row0=0, pose_xz=None, d_pos=3.0,
                                   d_neg=20.0, gt=None, rank=None, context=0, reverse="both"):
        """pair_threshold_counts on seq_filter(score_all_pairs(pooled_rows, pooled_cols)) without the matrix
        (sgpr_score_seq_threshold_counts): thresholds ascending float32, at most MAX_POOLED_THRESHOLDS.
        Returns (counts int64 [T+1], skipped, rank_sum or None), equal to pair_threshold_counts' on that matrix."""
        rows = self._pooled(pooled_rows, "pooled_rows")
        cols = self._pooled(pooled_cols, "pooled_cols")
        r, m = rows.shape[0], cols.shape[0]
        pose_xz, gt = self._truth(r, m, row0, pose_xz, gt, context)
        flags = self._flags(reverse=reverse)
        return self._threshold_counts(self.lib.sgpr_score_seq_threshold_counts,
                                      (self._h, _ptr(rows), r, _ptr(cols), m, int(context), int(seq_len), flags, int(row0),
                                       _ptr(pose_xz), float(d_pos), float(d_neg), _ptr(gt), m), thresholds, rank,
                                      lambda t: self.lib.sgpr_score_seq_threshold_counts_workspace_bytes(
                                          self._h, r, m, int(context), int(seq_len), flags, t))

    def forward_dense(self, features_1, features_2, k, want_att=True):
        """Drop-in SG.forward on dense [B,3+L,N] inputs -> (score [B], att1 [B,N], att2 [B,N])."""
        f1 = self._dev(features_1, torch.float32, "features_1")
        f2 = self._dev(features_2, torch.float32, "features_2")
        if f1.shape != f2.shape:
            raise ValueError("features_1 / features_2 shapes differ")
        b, ch, n = f1.shape
        if ch != 3 + self.dims.num_labels:
            raise ValueError("features must be [B, %d, N]" % (3 + self.dims.num_labels))
        score = torch.empty(b, dtype=torch.float32, device=self.device)
        att = torch.empty(2, b, n, dtype=torch.float32, device=self.device) if want_att else None
        ws_bytes = self.lib.sgpr_forward_workspace_bytes(self._h, b, n, k)
        ws = self._ws(ws_bytes)
        rc = self.lib.sgpr_forward_dense(self._h, _ptr(f1), _ptr(f2), b, n, k, _ptr(score),
                                         _ptr(att[0]) if want_att else None, _ptr(att[1]) if want_att else None,
                                         _ptr(ws), ws_bytes, self._stream())
        self._check(rc)
        if want_att:
            return score, att[0], att[1]
        return score, None, None


class PairPlan:
    """A pair list grouped by row graph (include/sgpr.h, sgpr_pair_plan): built on the host once, kept on the device."""

    def __init__(self, engine, idx1, idx2, num_rows, num_cols):
        i1 = np.ascontiguousarray(np.asarray(idx1).reshape(-1), dtype=np.int32)
        i2 = np.ascontiguousarray(np.asarray(idx2).reshape(-1), dtype=np.int32)
        if i1.size != i2.size:
            raise ValueError("pair sides differ in length: %d vs %d" % (i1.size, i2.size))
        lib = engine.lib
        self.P, self.num_rows, self.num_cols = int(i1.size), int(num_rows), int(num_cols)
        cap = int(lib.sgpr_pair_plan_ints(self.P, self.num_rows))
        words = np.empty(max(cap, 1), dtype=np.int32)
        used, nr, ni = ctypes.c_size_t(), ctypes.c_int32(), ctypes.c_int32()
        rc = lib.sgpr_pair_plan(i1.ctypes.data_as(ctypes.c_void_p), i2.ctypes.data_as(ctypes.c_void_p), self.P,
                                self.num_rows, self.num_cols, words.ctypes.data_as(ctypes.c_void_p), words.size,
                                ctypes.byref(used), ctypes.byref(nr), ctypes.byref(ni))
        _check(rc)
        self.n_rows, self.n_items = int(nr.value), int(ni.value)
        self.host_words = words[:int(used.value)]
        self.words = torch.from_numpy(self.host_words.copy()).to(engine.device)


# ---------------------------------------------------------------------- handle-free entry points (stand-alone modules)
def _gpu_f32(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s must be a tensor on the MI355X (there is no CPU fallback)" % name)
    return _on(t.detach(), t.device, torch.float32)


def knn(x, k):
    """dgcnn.knn (dgcnn.py:14-20): x [B,C,N] on the GPU -> idx [B,N,k] int64."""
    lib = load_library()
    x = _gpu_f32(x, "x")
    b, c, n = x.shape
    idx = torch.empty(b, n, int(k), dtype=torch.int64, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib.sgpr_knn(_ptr(x), b, c, n, int(k), _ptr(idx), _stream(x.device)))
    return idx


def graph_feature(x, idx):
    """dgcnn.get_graph_feature's gather (dgcnn.py:30-49): x [B,C,N], idx [B,N,k] int64 -> [B,2C,N,k]."""
    lib = load_library()
    x = _gpu_f32(x, "x")
    b, c, n = x.shape
    idx = idx.to(device=x.device, dtype=torch.int64).contiguous()
    if idx.shape[:2] != (b, n):
        raise ValueError("idx must be [B, N, k], got %s" % (tuple(idx.shape),))
    k = idx.shape[2]
    out = torch.empty(b, 2 * c, n, k, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib.sgpr_graph_feature(_ptr(x), _ptr(idx), b, c, n, k, _ptr(out), _stream(x.device)))
    return out


ATTENTION_MAX_NODES = 12288     # sgpr_attention_pool keeps a graph's N scores in 48 KB of LDS


def attention_pool(weight, emb):
    """AttentionModule.forward (layers_batch.py:28-39): weight [32,32], emb [B,N,32] -> (rep [B,32], att [B,N])."""
    lib = load_library()
    emb = _gpu_f32(emb, "embedding")
    weight = _gpu_f32(weight, "weight_matrix").to(emb.device)
    b, n, f = emb.shape
    if tuple(weight.shape) != (f, f):
        raise ValueError("attention_pool: weight_matrix must be [%d, %d]" % (f, f))
    # wider than the built module, or more nodes than its LDS holds scores for: the any-width kernel (plain fp32)
    if f > F3 or n > ATTENTION_MAX_NODES:
        rep = torch.empty(b, f, dtype=torch.float32, device=emb.device)
        att = torch.empty(b, n, dtype=torch.float32, device=emb.device)
        with torch.cuda.device(emb.device):
            _check(lib.sgpr_attention_pool_any(_ptr(weight), _ptr(emb), b, n, f, _ptr(rep), _ptr(att), _stream(emb.device)))
        return rep, att
    if f < F3:          # a smaller width is the built one with zero channels (exactly: zeros add nothing to any sum)
        emb = torch.nn.functional.pad(emb, (0, F3 - f))
        weight = torch.nn.functional.pad(weight, (0, F3 - f, 0, F3 - f))
    rep = torch.empty(b, F3, dtype=torch.float32, device=emb.device)
    att = torch.empty(b, n, dtype=torch.float32, device=emb.device)
    with torch.cuda.device(emb.device):
        _check(lib.sgpr_attention_pool(_ptr(weight), _ptr(emb), b, n, _ptr(rep), _ptr(att), _stream(emb.device)))
    return rep[:, :f], att


def ntn(weight, weight_block, bias, e1, e2):
    """TenorNetworkModule.forward (layers_batch.py:70-83): e1, e2 [B,32] -> [B,16]."""
    lib = load_library()
    e1 = _gpu_f32(e1, "embedding_1")
    e2 = _gpu_f32(e2, "embedding_2").to(e1.device)
    w = _gpu_f32(weight, "weight_matrix").to(e1.device)
    wb = _gpu_f32(weight_block, "weight_matrix_block").to(e1.device)
    bs = _gpu_f32(bias, "bias").to(e1.device).view(-1)
    b = e1.shape[0]
    f, t = (int(w.shape[0]), int(w.shape[2])) if w.dim() == 3 else (-1, -1)
    if (f < 1 or t < 1 or e1.shape != (b, f) or e2.shape != (b, f) or tuple(w.shape) != (f, f, t) or
            tuple(wb.shape) != (t, 2 * f) or bs.numel() != t):
        raise ValueError("ntn: weight_matrix [F,F,T], weight_matrix_block [T,2F], bias [T], embeddings [B,F]")
    if f > F3 or t > 16:   # wider than the built module: the any-width kernel (plain fp32)
        out = torch.empty(b, t, dtype=torch.float32, device=e1.device)
        with torch.cuda.device(e1.device):
            _check(lib.sgpr_ntn_any(_ptr(w.contiguous()), _ptr(wb.contiguous()), _ptr(bs.contiguous()), _ptr(e1),
                                    _ptr(e2), b, f, t, _ptr(out), _stream(e1.device)))
        return out
    if f < F3 or t < 16:   # a smaller module is the built one with zero weights for what it does not have
        pad = torch.nn.functional.pad
        e1, e2 = pad(e1, (0, F3 - f)).contiguous(), pad(e2, (0, F3 - f)).contiguous()
        w = pad(w, (0, 16 - t, 0, F3 - f, 0, F3 - f)).contiguous()
        wb = pad(torch.cat((pad(wb[:, :f], (0, F3 - f)), pad(wb[:, f:], (0, F3 - f))), dim=1), (0, 0, 0, 16 - t)).contiguous()
        bs = pad(bs, (0, 16 - t)).contiguous()
    out = torch.empty(b, 16, dtype=torch.float32, device=e1.device)
    with torch.cuda.device(e1.device):
        _check(lib.sgpr_ntn(_ptr(w), _ptr(wb), _ptr(bs), _ptr(e1), _ptr(e2), b, _ptr(out), _stream(e1.device)))
    return out[:, :t]


# struct sgpr_verify_result of include/sgpr.h (88 bytes, no padding) and its flag bits
VERIFY_RESULT = np.dtype([("inliers", "<i4"), ("inliers_refined", "<i4"), ("base", "<i4", (4,)), ("hypotheses", "<u4"),
                          ("flags", "<u4"), ("coarse", "<f4", (4,)), ("refined", "<f8", (4,)), ("rmse", "<f8")])
VERIFY_MAX_NODES = _C["SGPR_VERIFY_MAX_NODES"]
VERIFY_INVALID_INDEX, VERIFY_NO_HYPOTHESIS, VERIFY_TRUNCATED, VERIFY_NONFINITE = (
    _C["SGPR_VERIFY_" + name] for name in ("INVALID_INDEX", "NO_HYPOTHESIS", "TRUNCATED", "NONFINITE"))


def _verify_graphs(centers, labels, device, name):
    c, lab = _on(centers, device, torch.float32), _on(labels, device, torch.int32)
    if c.dim() != 3 or c.shape[2] != 3 or tuple(lab.shape) != tuple(c.shape[:2]):
        raise ValueError("%s: centers [G, N, 3] and labels [G, N]" % name)
    return c, lab


def verify_pairs(centers_a, labels_a, centers_b, labels_b, idx_a, idx_b, tau_edge=0.5, tau_inlier=0.6, tau_z=1.0,
                 min_base=5.0, max_hyp=65536, device=None):
    """sgpr_verify_pairs: geometric verification of the candidate pairs (idx_a[p], idx_b[p]) - planar consensus between
    the labelled centres of row graph idx_a[p] of (centers_a [GA,N,3], labels_a [GA,N]) and column graph idx_b[p] of
    (centers_b, labels_b).  Returns a dict of device tensors, one per field of the record (inliers, inliers_refined i32
    [P]; base i32 [P,4]; hypotheses i64 [P]; flags i32 [P]; coarse f32 [P,4]; refined f64 [P,4]; rmse f64 [P]), plus
    yaw = atan2(s, c) of the refined transform (f64 [P], radians) and record, the raw bytes u8 [P,88]
    (VERIFY_RESULT).  An index outside its graph set (-1: a padding slot of a top-k list) gives a zeroed record with
    VERIFY_INVALID_INDEX.  Asynchronous on the current stream."""
    lib = load_library()
    if device is None:
        device = _device_of(centers_a, centers_b, idx_a, idx_b)
    ca, la = _verify_graphs(centers_a, labels_a, device, "row graphs")
    cb, lb = _verify_graphs(centers_b, labels_b, device, "column graphs")
    if ca.shape[1] != cb.shape[1]:
        raise ValueError("verify_pairs: both graph sets must have the same number of slots per graph")
    ia, ib = _on(idx_a, device, torch.int32).view(-1), _on(idx_b, device, torch.int32).view(-1)
    if ia.numel() != ib.numel():
        raise ValueError("verify_pairs: idx_a and idx_b must have the same length")
    p = ia.numel()
    rec = torch.empty(p, VERIFY_RESULT.itemsize, dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        _check(lib.sgpr_verify_pairs(_ptr(ca), _ptr(la), ca.shape[0], _ptr(cb), _ptr(lb), cb.shape[0], ca.shape[1],
                                     _ptr(ia), _ptr(ib), p, float(tau_edge), float(tau_inlier), float(tau_z),
                                     float(min_base), int(max_hyp), _ptr(rec), _stream(rec.device)))
    return verify_fields(rec)


def verify_fields(rec):
    """The fields of sgpr_verify_result records (u8 [P,88] on any device) as tensors + yaw of the refined transform."""
    i32, f32v, f64v = rec.view(torch.int32), rec.view(torch.float32), rec.view(torch.float64)
    refined = f64v[:, 6:10]
    return {"inliers": i32[:, 0], "inliers_refined": i32[:, 1], "base": i32[:, 2:6],
            "hypotheses": i32[:, 6].to(torch.int64) & 0xffffffff, "flags": i32[:, 7], "coarse": f32v[:, 8:12],
            "refined": refined, "rmse": f64v[:, 10], "yaw": torch.atan2(refined[:, 1], refined[:, 0]), "record": rec}


CONSISTENCY_MAX_CLOSURES = _C["SGPR_CONSISTENCY_MAX_CLOSURES"]
CONSISTENCY_MAX_GROUPS = _C["SGPR_CONSISTENCY_MAX_GROUPS"]


def closure_consistency(rows, cols, T, Xr, Xc, group, n_groups, max_trans, min_cos, lever_gain, device=None):
    """sgpr_closure_consistency: which of the C closures (rows[p], cols[p], T[p] f64 [C,4] = the refined
    transform of verify_pairs) agree pair by pair through the planar odometry Xr [MR,4] / Xc [MC,4] (c, s, x, y; f64),
    within a group (group i32 [C], 0..n_groups-1).  min_cos is the cosine of the yaw tolerance.
    -> (adj i64 [C, ceil(C/64)]: bit q & 63 of word q >> 6 of row p, degree i32 [C], members i32 [C] = the group of every
    closure that is not void, -1 of a void one: what consistent_set takes).  Device tensors, asynchronous on the current
    stream."""
    lib = load_library()
    if device is None:
        device = _device_of(T, rows, cols, Xr, Xc, group)
    r, c, g = (_on(t, device, torch.int32).view(-1) for t in (rows, cols, group))
    t = _on(T, device, torch.float64).view(-1, 4)
    xr, xc = _on(Xr, device, torch.float64).view(-1, 4), _on(Xc, device, torch.float64).view(-1, 4)
    n = r.numel()
    if c.numel() != n or g.numel() != n or t.shape[0] != n:
        raise ValueError("closure_consistency: rows, cols, group and T must describe the same number of closures")
    adj = torch.empty(n, (n + 63) // 64, dtype=torch.int64, device=device)
    degree = torch.empty(n, dtype=torch.int32, device=device)
    need = int(lib.sgpr_closure_consistency_workspace_bytes(n)) if 0 <= n <= CONSISTENCY_MAX_CLOSURES else 0
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        _check(lib.sgpr_closure_consistency(_ptr(r), _ptr(c), _ptr(t), n, _ptr(xr), xr.shape[0], _ptr(xc),
                                            xc.shape[0], _ptr(g), int(n_groups), float(max_trans), float(min_cos),
                                            float(lever_gain), _ptr(adj), _ptr(degree), _ptr(ws), need,
                                            _stream(adj.device)))
    return adj, degree, ws[:4 * n].view(torch.int32)


def consistent_set(adj, group, n_groups, device=None):
    """sgpr_consistent_set: the greedy clique of every group on a bit matrix adj i64 [C, ceil(C/64)] (closure_consistency's,
    or any other: diagonal bits and bits beyond C are ignored) -> (rank i32 [C]: the order in which the closure was chosen
    within its group, -1 = not selected; group_size i32 [n_groups]).  group i32 [C]: outside 0..n_groups-1 = in no group.
    Device tensors, asynchronous on the current stream."""
    lib = load_library()
    if device is None:
        device = adj.device if isinstance(adj, torch.Tensor) and adj.is_cuda else torch.device("cuda", torch.cuda.current_device())
    g = _on(group, device, torch.int32).view(-1)
    n = g.numel()
    a = _on(adj, device, torch.int64)
    if a.numel() != n * ((n + 63) // 64):
        raise ValueError("consistent_set: adj must be [C, ceil(C/64)] for the C entries of group")
    rank = torch.empty(n, dtype=torch.int32, device=device)
    size = torch.empty(max(int(n_groups), 0), dtype=torch.int32, device=device)
    need = int(lib.sgpr_consistent_set_workspace_bytes(n)) if 0 <= n <= CONSISTENCY_MAX_CLOSURES else 0
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        _check(lib.sgpr_consistent_set(_ptr(a), n, _ptr(g), int(n_groups), _ptr(rank), _ptr(size), _ptr(ws), need,
                                       _stream(rank.device)))
    return rank, size


def cluster_scan(points, labels, max_nodes=1024, want_point_node=False):
    """sgpr_cluster_scan: points [P, >=3] f32 and raw labels [P] (u32 bit pattern) on the GPU ->
    (centers float64 [n,3], node labels int32 [n], cluster sizes int32 [n], point -> node int32 [P] or None)."""
    lib = load_library()
    points = _gpu_f32(points, "points")
    p, stride = points.shape
    labels = labels.to(points.device).contiguous()
    if labels.dtype not in (torch.int32, torch.uint32) or labels.numel() != p:
        raise ValueError("labels must be [P] int32 / uint32 (the raw .label words)")
    dev = points.device
    centers = torch.zeros(max_nodes, 3, dtype=torch.float64, device=dev)
    nlab = torch.zeros(max_nodes, dtype=torch.int32, device=dev)
    nsize = torch.zeros(max_nodes, dtype=torch.int32, device=dev)
    pnode = torch.empty(p, dtype=torch.int32, device=dev) if want_point_node else None
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    ws_bytes = lib.sgpr_cluster_workspace_bytes(p)
    ws = torch.empty(max(int(ws_bytes), 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(lib.sgpr_cluster_scan(_ptr(points), stride, _ptr(labels), p, max_nodes, _ptr(centers), _ptr(nlab),
                                     _ptr(nsize), _ptr(pnode), _ptr(count), _ptr(ws), ws_bytes, _stream(points.device)))
    n = int(count.item())
    if n < 0 or n > max_nodes:
        raise SgprError(-3, "scan produced %s nodes, more than max_nodes=%d" % ("> 8192" if n < 0 else n, max_nodes))
    return centers[:n], nlab[:n], nsize[:n], pnode


def graph_edges(points, point_node, centers):
    """sgpr_graph_edges: the pairwise "closest points near the midpoint" distances of gen_graphs -> float64 [n, n]."""
    lib = load_library()
    points = points.detach().to(torch.float32).contiguous()
    p, stride = points.shape
    n = centers.shape[0]
    dev = points.device
    out = torch.zeros(n, n, dtype=torch.float64, device=dev)
    if n == 0:
        return out
    ws = torch.empty(n * n * 4, dtype=torch.uint8, device=dev)
    centers = centers.to(device=dev, dtype=torch.float64).contiguous()
    point_node = point_node.to(device=dev, dtype=torch.int32).contiguous()
    with torch.cuda.device(dev):
        _check(lib.sgpr_graph_edges(_ptr(points), stride, _ptr(point_node), p, n, _ptr(centers), _ptr(out), _ptr(ws),
                                    n * n * 4, _stream(points.device)))
    return out
