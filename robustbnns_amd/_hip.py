"""ctypes binding of librbnn_hip.so (include/robustbnns_hip.h) — the only compute backend.

There is no CPU fallback: if the shared library is missing or a call fails, this raises.
torch is used for device memory and streams only; every kernel is launched through the C-ABI
with raw device pointers (`tensor.data_ptr()`) on torch's current HIP stream.
"""
import ctypes as C
import os

import torch          # must be imported first: the .so then binds to torch's already-loaded libamdhip64.so.7

from . import _header
from ._header import HipError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "librbnn_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "robustbnns_hip.h")

# Python class -> C struct.  Everything below — the ctypes.Structure classes, SIGNATURES, the constants and the *_KEYS — is generated from the
# header at import (_header.py), so a new entry point is an edit of the header, and of this mapping when it brings a struct.
STRUCTS = {
    "Posterior": "rbnn_posterior", "Workspace": "rbnn_workspace", "WorkspaceSizes": "rbnn_workspace_sizes",
    "ConvPosterior": "rbnn_conv_posterior", "ConvWorkspace": "rbnn_conv_workspace", "ConvWorkspaceSizes": "rbnn_conv_workspace_sizes",
    # rbnn_split_images has the same fields in the same order (two or three fp16 pieces per weight behind the pointers): one class for both
    "PieceImages": "rbnn_triple_images", "SplitImages": "rbnn_triple_images", "TripleImages": "rbnn_triple_images",
    "SplitWorkspace": "rbnn_split_workspace", "SplitWorkspaceSizes": "rbnn_split_workspace_sizes",
    "TripleWorkspace": "rbnn_triple_workspace", "TripleWorkspaceSizes": "rbnn_triple_workspace_sizes",
    "SviGuide": "rbnn_svi_guide", "SviFlatTensor": "rbnn_svi_flat_tensor", "SviTrainNet": "rbnn_svi_train_net", "SviTrainWs": "rbnn_svi_train_ws",
    "NnTrainNet": "rbnn_nn_train_net", "NnTrainWs": "rbnn_nn_train_ws",
    "ConvTrainNet": "rbnn_conv_train_net", "ConvTrainWs": "rbnn_conv_train_ws", "ConvTrainBytes": "rbnn_conv_train_bytes",
    "ConvSviTrainNet": "rbnn_conv_svi_train_net",
    "ConvEnsNet": "rbnn_conv_ens_net", "ConvEnsWs": "rbnn_conv_ens_ws", "ConvEnsBytes": "rbnn_conv_ens_bytes",
    "ConvSviLockstepNet": "rbnn_conv_svi_guides_net", "ConvSviLockstepWs": "rbnn_conv_svi_guides_ws", "ConvSviLockstepBytes": "rbnn_conv_svi_guides_bytes",
    "HmcChain": "rbnn_hmc_chain", "HmcLockstep": "rbnn_hmc_lockstep", "ConvHmcChainsNet": "rbnn_conv_hmc_chains_net", "SviLockstep": "rbnn_svi_multi", "SviLockstepAcc": "rbnn_svi_multi_acc",
}
HEADER = _header.read(HEADER_PATH)
# name -> (restype, argtypes) of every prototype of the header.  The pointer rule: `T *` / `const T *` with T a struct of STRUCTS is
# POINTER(its class), a returned `const char *` is c_char_p, every other pointer — rbnn_dev_scale (a device-side record the host never
# builds) and the scalar out-parameters included — is c_void_p, which takes byref(...), a c_void_p, an integer address and None.
_classes, SIGNATURES = _header.bind(HEADER, STRUCTS, same={"rbnn_split_images": "rbnn_triple_images"}, opaque=("rbnn_dev_scale",))
globals().update(_classes)
globals().update(HEADER.constants)          # RBNN_X of a #define or an enumerator is X here: CPAD, ABI_VERSION, OUT_*, LOSS_*, HMC_*, ...
SVI_LOCKSTEP_ACC_SAMPLES = HEADER.constants["SVI_MULTI_ACC_SAMPLES"]

ACTIVATIONS = {"relu": ACT_RELU, "leaky": ACT_LEAKY, "sigm": ACT_SIGM, "tanh": ACT_TANH}          # model_nn.py:66-75
ARCHS = {"fc": ARCH_FC, "fc2": ARCH_FC2}                                                          # model_nn.py:77-91
# rbnn_hmc.hip: the state block's indices
HMC_ST = {"eps": HMC_ST_EPS, "U": HMC_ST_U, "t": HMC_ST_T, "gbar": HMC_ST_GBAR, "xbar": HMC_ST_XBAR, "mu": HMC_ST_MU, "dH": HMC_ST_DH,
          "accept_prob": HMC_ST_ACC_PROB, "accepted": HMC_ST_ACCEPTED, "u": HMC_ST_UNIF, "U_new": HMC_ST_U_NEW, "K_new": HMC_ST_K_NEW,
          "K_old": HMC_ST_K_OLD}

_keys = lambda cls: tuple(name for name, _ in cls._fields_)
WS_KEYS, CONV_WS_KEYS, SPLIT_WS_KEYS, TRIPLE_WS_KEYS = _keys(Workspace), _keys(ConvWorkspace), _keys(SplitWorkspace), _keys(TripleWorkspace)
SVI_TRAIN_WS_KEYS, NN_TRAIN_WS_KEYS, CONV_TRAIN_WS_KEYS = _keys(SviTrainWs), _keys(NnTrainWs), _keys(ConvTrainWs)
CONV_ENS_WS_KEYS = _keys(ConvEnsWs)
CONV_SVI_LOCKSTEP_WS_KEYS = _keys(ConvSviLockstepWs)
SVI_LOCKSTEP_ACC_KEYS = _keys(SviLockstepAcc)
F64_WS_KEYS = ("P", "dZ", "Psum", "dact1", "hid1", "dact2")        # rbnn_f64_workspace_query's order (plain fp64 pointers: no struct)
assert len(F64_WS_KEYS) == F64_WS_BUFFERS
CONV_FP64_WS_KEYS = ("P", "dZ", "Psum", "P1", "arg1", "Q2", "arg2", "Gs")     # rbnn_conv_fp64_workspace_query's order; arg1 / arg2 are bytes
assert len(CONV_FP64_WS_KEYS) == CONV_FP64_WS_BUFFERS
CONV_WGRAD_DP_WS_KEYS = ("ce", "dO2", "dO1")                       # rbnn_conv_wgrad_dp_workspace_query's order: the weight-gradient checker's own buffers
assert len(CONV_WGRAD_DP_WS_KEYS) == CONV_WGRAD_DP_WS_BUFFERS
CONV_WGRAD_DP_OUT_KEYS = ("dK1w", "dK1b", "dK2w", "dK2b", "dFw", "dFb")     # rbnn_conv_weight_grads_dp's six outputs, in its order
FC_WGRAD_DP_WS_KEYS = ("ce", "hidL")                              # rbnn_fc_wgrad_dp_workspace_query's order: the fc / fc2 weight-gradient checker's own buffers
assert len(FC_WGRAD_DP_WS_KEYS) == FC_WGRAD_DP_WS_BUFFERS
FC_WGRAD_DP_OUT_KEYS = ("dW1", "db1", "dWm", "dbm", "dW2", "db2")  # rbnn_fc_weight_grads_dp's six outputs, in its order (dWm, dbm: fc2)

_lib = None


def load():
    """Load librbnn_hip.so (built by __graft_entry__.build()).  Raises if it is not there."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`. "
                           "robustbnns_amd has no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)            # AttributeError if the .so does not export a declared symbol
            fn.restype, fn.argtypes = res, args
        if lib.rbnn_abi_version() != ABI_VERSION:
            raise HipError(f"librbnn_hip.so ABI version {lib.rbnn_abi_version()} != {ABI_VERSION}: rebuild it (__graft_entry__.build())")
        flags = lib.rbnn_build_flags()
        if flags != 0 and os.environ.get("RBNN_ALLOW_ABLATION") != "1":
            raise HipError(f"librbnn_hip.so was built with timing-only ablation switches (rbnn_build_flags() = {flags}): its kernels compute "
                           "wrong results by design.  Rebuild it (`python __graft_entry__.py --force`); the scripts under tools/ that build "
                           "such variants set RBNN_ALLOW_ABLATION=1 for their own runs.")
        _lib = lib
    return _lib


def check(rc, what):
    if rc != 0:
        raise HipError(f"{what} failed: {load().rbnn_strerror(rc).decode()} ({rc})")


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def fill(rec, src):
    """The record `rec` (a Structure class: a new one of it) with its pointer fields set by name from `src`: a dict of tensors, or an object
    that holds them as attributes.  A name that is missing or None: NULL.  The other fields are left as they are."""
    rec = rec() if isinstance(rec, type) else rec
    get = src.get if isinstance(src, dict) else vars(src).get
    for k in rec._pointers_:
        setattr(rec, k, ptr(get(k)))
    return rec


def stream_of(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def require_gpu(t, name="tensor"):
    if t.device.type != "cuda":
        raise HipError(f"{name} is on {t.device}: the MI355X HIP kernels are the only compute path "
                       "(no CPU fallback); move it to 'cuda'.")
    if t.dtype != torch.float32 and t.dtype != torch.int32:
        raise HipError(f"{name} must be float32/int32, got {t.dtype}")
    if not t.is_contiguous():
        raise HipError(f"{name} must be contiguous")


class HipKernels:
    """Tensor-level façade over the C-ABI.  `net` is a robustbnns_amd.posterior.StackedPosterior,
    `ws` a dict of torch tensors keyed like rbnn_workspace."""

    name = "hip"

    def __init__(self):
        self.lib = load()

    # -- host-only --------------------------------------------------------------------------------
    def workspace_sizes(self, net, N, S, chunk=0):
        out = WorkspaceSizes()
        check(self.lib.rbnn_workspace_query(C.byref(net.descriptor(lazy_ok=True)), N, S, chunk, C.byref(out)), "rbnn_workspace_query")
        d = {k: getattr(out, k) for k in WS_KEYS}
        d["n_slabs"], d["chunk"] = out.n_slabs, out.chunk
        return d

    @staticmethod
    def _ws(ws):
        return fill(Workspace, ws)

    @staticmethod
    def _conv_ws(ws):
        return fill(ConvWorkspace, ws)

    # -- device -----------------------------------------------------------------------------------
    def fc_forward(self, net, X, sidx, S, out_kind, ws):
        require_gpu(X, "X")
        w = self._ws(ws)
        check(self.lib.rbnn_fc_forward(C.byref(net.descriptor()), ptr(X), X.stride(0), X.shape[0], ptr(sidx), S,
                                       out_kind, C.byref(w), stream_of(X)), "rbnn_fc_forward")

    def reduce_samples(self, P, S, N, Cn, scale, out):
        require_gpu(P, "P")
        check(self.lib.rbnn_reduce_samples(ptr(P), S, N, Cn, scale, ptr(out), out.stride(0), stream_of(P)), "rbnn_reduce_samples")

    def loss_dlogits(self, mode, P, Psum, G_up, labels, S, inv_S, N, Cn, dZ):
        require_gpu(P, "P")
        ldp = Psum.stride(0) if Psum is not None else (G_up.stride(0) if G_up is not None else CPAD)
        check(self.lib.rbnn_loss_dlogits(mode, ptr(P), ptr(Psum), ldp, ptr(G_up), ptr(labels), S, inv_S, N, Cn,
                                         ptr(dZ), stream_of(P)), "rbnn_loss_dlogits")

    def fc_input_grad(self, net, sidx, S, N, chunk, ws):
        w = self._ws(ws)
        n = C.c_int32(0)
        check(self.lib.rbnn_fc_input_grad(C.byref(net.descriptor()), ptr(sidx), S, N, chunk, C.byref(w), C.byref(n),
                                          stream_of(ws["dZ"])), "rbnn_fc_input_grad")
        return n.value

    def sum_slabs(self, slabs, K, N, Dp, scale, out):
        require_gpu(slabs, "slabs")
        check(self.lib.rbnn_sum_slabs(ptr(slabs), K, N, Dp, scale, ptr(out), out.stride(0), stream_of(slabs)), "rbnn_sum_slabs")

    def sum_slabs_norms(self, slabs, K, N, Dp, D, scale, out, linf, l2):
        """sum_slabs + per-point Linf / L2 norms of the result over the D real columns, one pass."""
        require_gpu(slabs, "slabs")
        check(self.lib.rbnn_sum_slabs_norms(ptr(slabs), K, N, Dp, D, scale, ptr(out), out.stride(0), ptr(linf), ptr(l2),
                                            stream_of(slabs)), "rbnn_sum_slabs_norms")

    def pgd_alpha(self, X0, D, alpha):
        require_gpu(X0, "X0")
        check(self.lib.rbnn_pgd_alpha(ptr(X0), X0.stride(0), X0.shape[0], D, ptr(alpha), stream_of(X0)), "rbnn_pgd_alpha")

    def attack_step(self, X, X0, G, K, slab_stride, ldg, alpha, alpha_scalar, eps, project, D):
        require_gpu(X, "X")
        check(self.lib.rbnn_attack_step(ptr(X), ptr(X0), X.stride(0), ptr(G), K, slab_stride, ldg, ptr(alpha),
                                        alpha_scalar, eps, int(project), X.shape[0], D, stream_of(X)), "rbnn_attack_step")

    def eval_metrics(self, A, B, labels, Cn, counts, rob):
        require_gpu(A, "outputs")
        check(self.lib.rbnn_eval_metrics(ptr(A), ptr(B), A.stride(0), ptr(labels), A.shape[0], Cn, ptr(counts), ptr(rob),
                                         stream_of(A)), "rbnn_eval_metrics")

    def pack_rows4(self, W, out):
        """[rows, cols] row-major -> [rows/4, cols, 4] (rows = leading dims of W flattened)."""
        require_gpu(W, "W")
        cols = W.shape[-1]
        check(self.lib.rbnn_pack_rows4(ptr(W), W.numel() // cols, cols, ptr(out), stream_of(W)), "rbnn_pack_rows4")

    # -- split-half ("f16x3") precision mode ---------------------------------------------------------
    def input_scales(self, X, cols, floor_abs, mul, add, cap, out):
        """Device-resident operand scales of the inputs X [N, ld] (record 0) and of the activations they bound (record 1):
        out = int32[8] on the device (two rbnn_dev_scale records).  No host sync."""
        require_gpu(X, "X")
        check(self.lib.rbnn_input_scales(ptr(X), X.shape[0], cols, X.stride(0), floor_abs, mul, add, cap, ptr(out), stream_of(X)),
              "rbnn_input_scales")
        return out

    # The wrappers of the two fp16-piece modes come in pairs with one body each; `name` is the mode's C function.
    def _rows_image(self, name, src, cols, scale_exp, out, ld_dst, dev_scale):
        require_gpu(src, "src")
        ld_src = src.shape[-1]
        check(getattr(self.lib, name)(ptr(src), src.numel() // ld_src, cols, ld_src, scale_exp, ptr(dev_scale), ptr(out), ld_dst, stream_of(src)), name)

    def _cols_image(self, name, W, rows, cols, scale_exp, out, ld_dst):
        require_gpu(W, "W")
        check(getattr(self.lib, name)(ptr(W), W.numel() // (rows * W.shape[-1]), rows, cols, W.shape[-1], scale_exp, ptr(out), ld_dst, stream_of(W)), name)

    def _w2gen_image(self, name, W2, Cn, H, scale_exp, out):
        require_gpu(W2, "W2")
        check(getattr(self.lib, name)(ptr(W2), W2.numel() // (Cn * H), Cn, H, scale_exp, ptr(out), stream_of(W2)), name)

    def _piece_workspace_sizes(self, name, out, desc, images, N, S):
        check(getattr(self.lib, name)(C.byref(desc), C.byref(images), N, S, C.byref(out)), name)
        return {k: getattr(out, k) for k, _ in out._fields_}

    def _fc_input_grad_pieces(self, name, desc, images, sidx, S, N, chunk, w, pw, stream):
        n = C.c_int32(0)
        check(getattr(self.lib, name)(C.byref(desc), C.byref(images), ptr(sidx), S, N, chunk, C.byref(w), C.byref(pw), C.byref(n), stream), name)
        return n.value

    def split_rows(self, src, cols, scale_exp, out, ld_dst, dev_scale=None):
        """src: [..., ld_src] fp32 rows -> out: split-rows image (int16 storage [rows, ld_dst*2]).  dev_scale: an
        rbnn_dev_scale record on the device that replaces scale_exp."""
        self._rows_image("rbnn_split_rows", src, cols, scale_exp, out, ld_dst, dev_scale)

    def fc_forward_split(self, net, images, Xs, ld, x_exp, N, sidx, S, out_kind, ws, dev_scales=None):
        w = self._ws(ws)
        check(self.lib.rbnn_fc_forward_split(C.byref(net.descriptor()), C.byref(images), ptr(Xs), ld, x_exp, ptr(dev_scales), N,
                                             ptr(sidx), S, out_kind, C.byref(w), stream_of(Xs)), "rbnn_fc_forward_split")

    def split_cols(self, W, rows, cols, scale_exp, out, ld_dst):
        """W: [n_mats, rows, ld_src] fp32 -> out: split-cols image."""
        self._cols_image("rbnn_split_cols", W, rows, cols, scale_exp, out, ld_dst)

    def split_w2gen(self, W2, Cn, H, scale_exp, out):
        self._w2gen_image("rbnn_split_w2gen", W2, Cn, H, scale_exp, out)

    def split_workspace_sizes(self, net, images, N, S):
        return self._piece_workspace_sizes("rbnn_split_workspace_query", SplitWorkspaceSizes(), net.descriptor(), images, N, S)

    def fc_input_grad_split(self, net, images, sidx, S, N, chunk, ws, sws):
        return self._fc_input_grad_pieces("rbnn_fc_input_grad_split", net.descriptor(), images, sidx, S, N, chunk, self._ws(ws),
                                          fill(SplitWorkspace, sws), stream_of(ws["dZ"]))

    # -- triple-split ("f16x6") mode: full-width fp32 operands on the f16 matrix pipe ---------------------
    def triple_rows(self, src, cols, scale_exp, out, ld_dst, dev_scale=None, grouped=False):
        """src: [..., ld_src] fp32 rows -> out: triple-rows image (int16 storage, 3 halves per element).  grouped=True: the fc forward's
        operand order (16-row groups, [3 pieces][16 rows][64 B] per K stage; out sized for ceil16(rows) rows)."""
        self._rows_image("rbnn_triple_rows_grouped" if grouped else "rbnn_triple_rows", src, cols, scale_exp, out, ld_dst, dev_scale)

    def triple_cols(self, W, rows, cols, scale_exp, out, ld_dst):
        self._cols_image("rbnn_triple_cols", W, rows, cols, scale_exp, out, ld_dst)

    def triple_w2gen(self, W2, Cn, H, scale_exp, out):
        self._w2gen_image("rbnn_triple_w2gen", W2, Cn, H, scale_exp, out)

    def triple_workspace_sizes(self, net, images, N, S):
        return self._piece_workspace_sizes("rbnn_triple_workspace_query", TripleWorkspaceSizes(), net.descriptor(lazy_ok=True), images, N, S)

    def fc_forward_triple(self, net, images, tws, x_exp, N, sidx, S, out_kind, ws, dev_scales=None):
        w, t = self._ws(ws), fill(TripleWorkspace, tws)
        # (lazy_ok: a pending images-only draw left the fp32 W1 / Wm stale, which the triple kernels never read)
        check(self.lib.rbnn_fc_forward_triple(C.byref(net.descriptor(lazy_ok=True)), C.byref(images), C.byref(t), x_exp, ptr(dev_scales), N,
                                              ptr(sidx), S, out_kind, C.byref(w), stream_of(tws["X_triple"])), "rbnn_fc_forward_triple")

    def step_tail_triple(self, mode, P, labels, S, inv_S, N, Cn, tws, Psum=None):
        """reduce over samples + loss + dZ generator image in one launch (rbnn_step_tail_triple); the fp32 dZ is not written."""
        require_gpu(P, "P")
        t = fill(TripleWorkspace, tws)
        check(self.lib.rbnn_step_tail_triple(mode, ptr(P), ptr(labels), S, inv_S, N, Cn, ptr(Psum), 0 if Psum is None else Psum.stride(0), C.byref(t),
                                             stream_of(P)), "rbnn_step_tail_triple")

    def attack_step_triple(self, X, X0, G, K, slab_stride, ldg, alpha, alpha_scalar, eps, project, D, dev_scale, X_triple, ld_rows):
        """attack_step + the grouped triple-rows image of the new iterate in one launch (rbnn_attack_step_triple)."""
        require_gpu(X, "X")
        check(self.lib.rbnn_attack_step_triple(ptr(X), ptr(X0), X.stride(0), ptr(G), K, slab_stride, ldg, ptr(alpha), alpha_scalar, eps, int(project),
                                               X.shape[0], D, ptr(dev_scale), ptr(X_triple), ld_rows, stream_of(X)), "rbnn_attack_step_triple")

    def fc_input_grad_triple(self, net, images, sidx, S, N, chunk, ws, tws, dz_ready=False):
        """dz_ready: tws['dZ_gen'] / tws['g_scale'] were built by step_tail_triple — the fp32 dZ is not read."""
        w = self._ws(ws)
        if dz_ready:
            w.dZ = None
        return self._fc_input_grad_pieces("rbnn_fc_input_grad_triple", net.descriptor(lazy_ok=True), images, sidx, S, N, chunk, w,
                                          fill(TripleWorkspace, tws), stream_of(ws["slabs"]))

    # -- fp64 mode (rbnn_fp64.inc): fp32 data widened on load, every operation in fp64 --------------------
    def f64_workspace_sizes(self, net, N, S):
        out = (C.c_size_t * F64_WS_BUFFERS)()
        check(self.lib.rbnn_f64_workspace_query(C.byref(net.descriptor(lazy_ok=True)), N, S, out), "rbnn_f64_workspace_query")
        return dict(zip(F64_WS_KEYS, out))

    def fc_forward_f64(self, net, X, sidx, S, out_kind, ws):
        """ws: dict of float64 tensors keyed like F64_WS_KEYS.  (descriptor(): a pending images-only SVI draw is completed — this mode
        reads the fp32 weight stack.)"""
        require_gpu(X, "X")
        check(self.lib.rbnn_fc_forward_f64(C.byref(net.descriptor()), ptr(X), X.stride(0), X.shape[0], ptr(sidx), S, out_kind, ptr(ws["P"]),
                                           ptr(ws["dact1"]), ptr(ws.get("hid1")), ptr(ws.get("dact2")), stream_of(X)), "rbnn_fc_forward_f64")

    def reduce_samples_f64(self, P, S, N, Cn, scale, out):
        check(self.lib.rbnn_reduce_samples_f64(ptr(P), S, N, Cn, scale, ptr(out), out.stride(0), stream_of(P)), "rbnn_reduce_samples_f64")

    def loss_dlogits_f64(self, mode, P, Psum, labels, S, inv_S, N, Cn, dZ):
        check(self.lib.rbnn_loss_dlogits_f64(mode, ptr(P), ptr(Psum), CPAD, ptr(labels), S, inv_S, N, Cn, ptr(dZ), stream_of(P)),
              "rbnn_loss_dlogits_f64")

    def fc_input_grad_f64(self, net, sidx, S, N, ws, scale, G, linf=None, l2=None):
        check(self.lib.rbnn_fc_input_grad_f64(C.byref(net.descriptor()), ptr(sidx), S, N, ptr(ws["dZ"]), ptr(ws["dact1"]), ptr(ws.get("dact2")),
                                              scale, ptr(G), G.stride(0), ptr(linf), ptr(l2), stream_of(G)), "rbnn_fc_input_grad_f64")

    def attack_step_f64(self, X, X0, G, alpha, alpha_scalar, eps, project, D):
        require_gpu(X, "X")
        check(self.lib.rbnn_attack_step_f64(ptr(X), ptr(X0), X.stride(0), ptr(G), G.stride(0), ptr(alpha), alpha_scalar, eps, int(project),
                                            X.shape[0], D, stream_of(X)), "rbnn_attack_step_f64")

    # -- fp64 checker of the conv nets (rbnn_conv_fp64.inc); reduce_samples_f64 / loss_dlogits_f64 / attack_step_f64 above serve it too ----
    def conv_fp64_workspace_sizes(self, net, N, S):
        out = (C.c_size_t * CONV_FP64_WS_BUFFERS)()
        check(self.lib.rbnn_conv_fp64_workspace_query(C.byref(net.descriptor()), N, S, out), "rbnn_conv_fp64_workspace_query")
        return dict(zip(CONV_FP64_WS_KEYS, out))

    def conv_forward_fp64(self, net, X, sidx, S, out_kind, ws):
        """ws: dict keyed like CONV_FP64_WS_KEYS (float64 tensors; arg1 / arg2 uint8)."""
        require_gpu(X, "X")
        check(self.lib.rbnn_conv_forward_fp64(C.byref(net.descriptor()), ptr(X), X.stride(0), X.shape[0], ptr(sidx), S, out_kind, ptr(ws["P"]),
                                              ptr(ws["P1"]), ptr(ws["arg1"]), ptr(ws["Q2"]), ptr(ws["arg2"]), stream_of(X)), "rbnn_conv_forward_fp64")

    def conv_input_grad_fp64(self, net, sidx, S, N, ws, scale, G, linf=None, l2=None):
        check(self.lib.rbnn_conv_input_grad_fp64(C.byref(net.descriptor()), ptr(sidx), S, N, ptr(ws["dZ"]), ptr(ws["P1"]), ptr(ws["arg1"]),
                                                 ptr(ws["Q2"]), ptr(ws["arg2"]), ptr(ws["Gs"]), scale, ptr(G), G.stride(0), ptr(linf), ptr(l2),
                                                 stream_of(G)), "rbnn_conv_input_grad_fp64")

    # -- ... and of the conv weight gradients (rbnn_conv_wgrad_dp.inc): behind conv_forward_fp64 with logits out ---------------------------
    def conv_wgrad_dp_workspace_sizes(self, net, N, S):
        out = (C.c_size_t * CONV_WGRAD_DP_WS_BUFFERS)()
        check(self.lib.rbnn_conv_wgrad_dp_workspace_query(C.byref(net.descriptor()), N, S, out), "rbnn_conv_wgrad_dp_workspace_query")
        return dict(zip(CONV_WGRAD_DP_WS_KEYS, out))

    def conv_head_ce_dp(self, Z, labels, S, N, Cn, scale, dZ, ce):
        """Z, dZ [S, N, 16] float64, labels int32 [N] in [0, Cn), ce [S, N] float64."""
        check(self.lib.rbnn_conv_head_ce_dp(ptr(Z), ptr(labels), S, N, Cn, scale, ptr(dZ), ptr(ce), stream_of(Z)), "rbnn_conv_head_ce_dp")

    def conv_weight_grads_dp(self, net, X, sidx, S, ws, out):
        """ws: the forward's workspace and the three buffers of CONV_WGRAD_DP_WS_KEYS in one dict; out: float64 tensors keyed like
        CONV_WGRAD_DP_OUT_KEYS, which the call ADDS to."""
        require_gpu(X, "X")
        check(self.lib.rbnn_conv_weight_grads_dp(C.byref(net.descriptor()), ptr(X), X.stride(0), ptr(sidx), S, X.shape[0], ptr(ws["dZ"]),
                                                 ptr(ws["P1"]), ptr(ws["arg1"]), ptr(ws["Q2"]), ptr(ws["arg2"]), ptr(ws["dO2"]), ptr(ws["dO1"]),
                                                 *(ptr(out[k]) for k in CONV_WGRAD_DP_OUT_KEYS), stream_of(X)), "rbnn_conv_weight_grads_dp")

    # -- ... and of the fc / fc2 weight gradients (rbnn_fc_wgrad_dp.inc): behind fc_forward_f64 with logits out, conv_head_ce_dp and
    #    fc_input_grad_f64 -----------------------------------------------------------------------------------------------------------------
    def fc_wgrad_dp_workspace_sizes(self, net, N, S):
        out = (C.c_size_t * FC_WGRAD_DP_WS_BUFFERS)()
        check(self.lib.rbnn_fc_wgrad_dp_workspace_query(C.byref(net.descriptor(lazy_ok=True)), N, S, out), "rbnn_fc_wgrad_dp_workspace_query")
        return dict(zip(FC_WGRAD_DP_WS_KEYS, out))

    def fc_hidden_dp(self, net, X, sidx, S, ws):
        """ws: the forward's workspace (hid1: fc2) and hidL, which is written: the activations of the last hidden layer."""
        require_gpu(X, "X")
        check(self.lib.rbnn_fc_hidden_dp(C.byref(net.descriptor()), ptr(X), X.stride(0), ptr(sidx), S, X.shape[0], ptr(ws.get("hid1")),
                                         ptr(ws["hidL"]), stream_of(X)), "rbnn_fc_hidden_dp")

    def fc_weight_grads_dp(self, net, X, S, ws, out):
        """ws: the forward's workspace after fc_input_grad_f64 (dZ, dact1, hid1, dact2) and hidL in one dict; out: float64 tensors keyed like
        FC_WGRAD_DP_OUT_KEYS (dWm, dbm: fc2 only), which the call ADDS to."""
        require_gpu(X, "X")
        check(self.lib.rbnn_fc_weight_grads_dp(C.byref(net.descriptor()), ptr(X), X.stride(0), S, X.shape[0], ptr(ws["dZ"]), ptr(ws["dact1"]),
                                               ptr(ws.get("hid1")), ptr(ws.get("dact2")), ptr(ws["hidL"]),
                                               *(ptr(out.get(k)) for k in FC_WGRAD_DP_OUT_KEYS), stream_of(X)), "rbnn_fc_weight_grads_dp")

    # -- posterior-predictive uncertainty (rbnn_predictive.inc): reads the P of any forward above --------------------------------------------
    PREDICTIVE_OUTPUTS = ("entropy", "expected_entropy", "mutual_information", "confidence", "agreement", "variance", "nll", "brier",
                          "prediction", "correct")                        # rbnn_predictive_stats' ten outputs, in its order

    def predictive_stats(self, P, Cn, labels, prefixes, out, lo=0):
        """P: [S, n, ld] float32 or float64 with stride(2) == 1 (a forward's workspace as it stands).  out: name -> [J, N] tensor (float64;
        prediction, correct int32; a name left out is not computed), of which columns lo .. lo + n are written: row j the figures of the
        first prefixes[j] samples."""
        if P.dtype not in (torch.float32, torch.float64) or P.dim() != 3 or (P.shape[2] > 1 and P.stride(2) != 1) or P.device.type != "cuda":
            raise HipError(f"predictive_stats takes a float32 / float64 [S, n, ld] tensor on the GPU with stride(2) == 1, not {P.dtype} "
                           f"{tuple(P.shape)} on {P.device}")
        some = next(iter(out.values()))
        pre = (C.c_int32 * len(prefixes))(*prefixes)
        outs = [None if out.get(k) is None else C.c_void_p(out[k].data_ptr() + lo * out[k].element_size()) for k in self.PREDICTIVE_OUTPUTS]
        check(self.lib.rbnn_predictive_stats(ptr(P), PREDICTIVE_DOUBLE if P.dtype == torch.float64 else PREDICTIVE_FLOAT, P.stride(0), P.stride(1),
                                             P.shape[0], P.shape[1], Cn, ptr(labels), pre, len(prefixes), some.stride(0), *outs, stream_of(P)),
              "rbnn_predictive_stats")

    # -- conv architecture ---------------------------------------------------------------------------
    def conv_workspace_sizes(self, net, N, S):
        out = ConvWorkspaceSizes()
        check(self.lib.rbnn_conv_workspace_query(C.byref(net.descriptor()), N, S, C.byref(out)), "rbnn_conv_workspace_query")
        return {k: getattr(out, k) for k in CONV_WS_KEYS}

    def conv_forward(self, net, X, sidx, S, out_kind, ws):
        require_gpu(X, "X")
        w = self._conv_ws(ws)
        check(self.lib.rbnn_conv_forward(C.byref(net.descriptor()), ptr(X), X.stride(0), X.shape[0], ptr(sidx), S, out_kind,
                                         C.byref(w), stream_of(X)), "rbnn_conv_forward")

    def conv_forward_split(self, net, K2_rows, k2_exp, p1_exp, X, sidx, S, out_kind, ws, p1_dev_scale=None):
        require_gpu(X, "X")
        w = self._conv_ws(ws)
        check(self.lib.rbnn_conv_forward_split(C.byref(net.descriptor()), ptr(K2_rows), k2_exp, p1_exp, ptr(p1_dev_scale), ptr(X),
                                               X.stride(0), X.shape[0],
                                               ptr(sidx), S, out_kind, C.byref(w), stream_of(X)), "rbnn_conv_forward_split")

    def conv_forward_triple(self, net, K2_triple, k2_exp, p1_exp, X, sidx, S, out_kind, ws, p1_dev_scale=None):
        require_gpu(X, "X")
        w = self._conv_ws(ws)
        check(self.lib.rbnn_conv_forward_triple(C.byref(net.descriptor()), ptr(K2_triple), k2_exp, p1_exp, ptr(p1_dev_scale), ptr(X),
                                                X.stride(0), X.shape[0], ptr(sidx), S, out_kind, C.byref(w), stream_of(X)),
              "rbnn_conv_forward_triple")

    def conv_input_grad_dense(self, net, K2_dense, k2_exp, fw_l1, sidx, S, N, ws):
        w = self._conv_ws(ws)
        check(self.lib.rbnn_conv_input_grad_dense(C.byref(net.descriptor()), ptr(K2_dense), k2_exp, fw_l1, ptr(sidx), S, N, C.byref(w),
                                                  stream_of(ws["dZ"])), "rbnn_conv_input_grad_dense")
        return S

    def conv_weight_images(self, K2w, S, H, k2_exp, rows=None, dense=None):
        """model.3.weight's forward (grouped tap-major rows) and dense conv2^T triple images from the fp32 stack in one launch."""
        require_gpu(K2w, "K2w")
        check(self.lib.rbnn_conv_weight_images(ptr(K2w), S, H, k2_exp, ptr(rows), ptr(dense), stream_of(K2w)), "rbnn_conv_weight_images")

    def conv_input_grad_split(self, net, K2_bwd, k2_exp, fw_l1, sidx, S, N, ws):
        w = self._conv_ws(ws)
        check(self.lib.rbnn_conv_input_grad_split(C.byref(net.descriptor()), ptr(K2_bwd), k2_exp, fw_l1, ptr(sidx), S, N, C.byref(w),
                                                  stream_of(ws["dZ"])), "rbnn_conv_input_grad_split")
        return S

    def conv_input_grad(self, net, sidx, S, N, ws):
        w = self._conv_ws(ws)
        check(self.lib.rbnn_conv_input_grad(C.byref(net.descriptor()), ptr(sidx), S, N, C.byref(w), stream_of(ws["dZ"])),
              "rbnn_conv_input_grad")
        return S                                                          # one "slab" per sample

    def svi_materialize(self, loc, scale_raw, eps, out):
        require_gpu(loc, "loc")
        check(self.lib.rbnn_svi_materialize(ptr(loc), ptr(scale_raw), ptr(eps), loc.numel(), eps.shape[0], ptr(out),
                                            stream_of(loc)), "rbnn_svi_materialize")

    def svi_draw_supported(self, net, with_triple_images):
        return bool(self.lib.rbnn_svi_draw_supported(C.byref(net.descriptor()), int(bool(with_triple_images))))

    def svi_draw(self, net, images, guide, S, key, draw_id, sample_keys=None, images_only=False):
        """One launch: samples [0, S) of the stacked posterior `net` and all its weight images redrawn IN PLACE from the guide
        (robustbnns_amd.posterior.SviGuide).  images: the posterior's TripleImages or None.  sample_keys: int64 device tensor [S].
        images_only (rbnn_svi_draw_images): W1 / Wm into the triple images only — their fp32 stack and pack_rows4 copies are skipped."""
        w1 = net.__dict__.get("_t_W1", None) if hasattr(net, "__dict__") else None
        w1 = net.W1 if w1 is None else w1
        require_gpu(w1, "W1")
        fn = self.lib.rbnn_svi_draw_images if images_only else self.lib.rbnn_svi_draw
        check(fn(C.byref(net.descriptor(lazy_ok=True)), None if images is None else C.byref(images), C.byref(guide.descriptor()), S,
                 ptr(sample_keys), C.c_uint64(key & 0xFFFFFFFFFFFFFFFF), C.c_uint32(draw_id & 0xFFFFFFFF),
                 stream_of(w1)), "rbnn_svi_draw_images" if images_only else "rbnn_svi_draw")

    # -- low-dimensional fc nets: the whole hot path in one launch (rbnn_lowdim.hip) -------------------------
    LOWDIM_FORWARD, LOWDIM_GRADIENT, LOWDIM_ATTACK = LOWDIM_FORWARD, LOWDIM_GRADIENT, LOWDIM_ATTACK

    def lowdim_supported(self, net):
        return bool(self.lib.rbnn_lowdim_supported(C.byref(net.descriptor(lazy_ok=True))))

    def lowdim_scratch_bytes(self, net, N, S):
        return int(self.lib.rbnn_lowdim_scratch_bytes(C.byref(net.descriptor(lazy_ok=True)), N, S))

    def lowdim_fused_draw_supported(self, net, N, S):
        return bool(self.lib.rbnn_lowdim_fused_draw_supported(C.byref(net.descriptor(lazy_ok=True)), N, S))

    def lowdim_run(self, net, op, loss_mode, out_kind, X, X0, sidx, S, labels, inv_S, out_scale, eps, alpha, alpha_scalar, alpha_per_image,
                   project, iters, P, out, linf=None, l2=None):
        require_gpu(X, "X")
        lazy = getattr(net, "_lazy", None)
        covered = sidx is None or getattr(sidx, "_rbnn_max_index", 1 << 62) < (lazy[2] if lazy is not None else 0)
        if (lazy is not None and getattr(net, "_triple", None) is None and covered and S <= lazy[2]
                and self.lowdim_fused_draw_supported(net, X.shape[0], S)):
            # a pending (lazy) SVI draw: the weights are generated inside this launch — no rbnn_svi_draw launch, the stack stays as it was.
            # Only when every sample the call names is one the draw covers: the identity map over the first S <= drawn samples, or an index
            # buffer whose largest index is KNOWN on the host (AttackEngine.sample_index records it) and below the drawn count — the kernel
            # reads sample_keys[sidx[s]].  Any other index buffer materialises the draw first (net.descriptor() below does) and reads the stack
            key, draw_id, _, sample_keys = lazy
            check(self.lib.rbnn_lowdim_run_svi(C.byref(net.descriptor(lazy_ok=True)), C.byref(net._guide.descriptor()), ptr(sample_keys),
                                               C.c_uint64(key & 0xFFFFFFFFFFFFFFFF), C.c_uint32(draw_id & 0xFFFFFFFF), op, loss_mode, out_kind, ptr(X),
                                               ptr(X0), X.stride(0), X.shape[0], ptr(sidx), S, ptr(labels), inv_S, out_scale, eps, ptr(alpha), alpha_scalar,
                                               int(alpha_per_image), int(project), iters, ptr(P), ptr(out), out.stride(0), ptr(linf), ptr(l2),
                                               stream_of(X)), "rbnn_lowdim_run_svi")
            return
        check(self.lib.rbnn_lowdim_run(C.byref(net.descriptor()), op, loss_mode, out_kind, ptr(X), ptr(X0), X.stride(0), X.shape[0], ptr(sidx), S,
                                       ptr(labels), inv_S, out_scale, eps, ptr(alpha), alpha_scalar, int(alpha_per_image), int(project), iters,
                                       ptr(P), ptr(out), out.stride(0), ptr(linf), ptr(l2), stream_of(X)), "rbnn_lowdim_run")

    def svi_draw_flat(self, items, S, key, draw_id, sample_keys=None):
        """items: list of (loc, sigma = softplus(raw scale), out [S, ...], tensor_id) — every tensor of a net redrawn in place by ONE launch."""
        arr = (SviFlatTensor * len(items))()
        for i, (loc, scl, out, tid) in enumerate(items):
            require_gpu(out, "out")
            arr[i].loc, arr[i].sigma, arr[i].out = loc.data_ptr(), scl.data_ptr(), out.data_ptr()
            arr[i].n_elem, arr[i].out_sample_stride, arr[i].tensor_id = loc.numel(), out.stride(0), tid
        check(self.lib.rbnn_svi_draw_flat(arr, len(items), S, ptr(sample_keys), C.c_uint64(key & 0xFFFFFFFFFFFFFFFF), C.c_uint32(draw_id & 0xFFFFFFFF),
                                          stream_of(items[0][2])), "rbnn_svi_draw_flat")
