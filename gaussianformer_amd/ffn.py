"""The encoder's feed-forward block: drop-in for ``AsymmetricFFN`` (model/encoder/gaussian_encoder/ffn_module.py:8-75) and the
one-launch form of the ``"ffn", "norm"`` and ``"identity", "ffn", "add", "norm"`` runs of the encoder's ``operation_order``.
torch runs a block as two LayerNorms, three GEMMs, a ReLU and an add around an ``[A, 512]`` hidden tensor;
``gf_ffn_forward`` (include/gf_hip.h) is one launch in which the hidden row never reaches memory.  The
training step -- the module's two dropouts, a saving forward and the full backward (``gf_ffn_forward_train``,
``gf_ffn_backward``) -- is ``ffn_block_autograd`` and, on the module, the opt-in ``native_training``; without
it training, dropout and everything the native op does not cover run the module's own torch layers."""
import torch
import torch.nn as nn

from . import _lib

f32 = torch.float32
E_NATIVE, F_NATIVE, CIN_NATIVE = _lib.GF_FFN_EMBED_DIMS, _lib.GF_FFN_HIDDEN, (128, 256)
# the library's table order: state_dict keys of the module, then the post norm's pair
_KEYS = ("pre_norm.weight", "pre_norm.bias", "layers.0.0.weight", "layers.0.0.bias", "layers.1.weight", "layers.1.bias",
         "identity_fc.weight", "identity_fc.bias")


def _param_list(ffn, norm):
    """The 10 parameters in the library's order (``None`` for an absent part), from a module with the reference's submodule
    names or a mapping with its state_dict keys, and the post norm (an ``nn.LayerNorm``, a ``(weight, bias)`` pair or ``None``)."""
    if isinstance(ffn, nn.Module):
        def get(key):
            obj = ffn
            for name in key.split("."):
                obj = obj[int(name)] if name.isdigit() else getattr(obj, name, None)
                if obj is None:
                    return None
            return obj
        for name in ("pre_norm", "identity_fc"):   # an nn.Identity has no weight: absent
            sub = getattr(ffn, name, None)
            if sub is not None and not isinstance(sub, (nn.LayerNorm, nn.Linear, nn.Identity)):
                raise ValueError(f"ffn_block: {name} is a {type(sub).__name__}, not a LayerNorm / Linear")
        if getattr(ffn, "add_identity", False) and isinstance(getattr(ffn, "identity_fc", None), nn.Identity):
            raise ValueError("ffn_block: an identity_fc that is nn.Identity (feedforward_channels == embed_dims) has no native form")
        if not isinstance(getattr(ffn, "activate", nn.ReLU()), nn.ReLU) or len(ffn.layers) != 3:
            raise ValueError("ffn_block: the native block is Linear, ReLU, Linear (num_fcs = 2)")
        params = [get(k) for k in _KEYS]
    else:
        params = [ffn.get(k) for k in _KEYS]
    return [*params, *_lib.norm_pair(norm, "ffn_block")]


def _shape(x, params, residual):
    """``(x [n, Cin], residual [n, E] or None, leading shape, Cin, F, E)`` as the library reads them, the shapes checked."""
    _lib.require_gpu(x, residual, *params)
    w1, w2 = params[2], params[4]
    if w1 is None or w2 is None or params[3] is None or params[5] is None:
        raise ValueError("ffn_block needs layers.0.0 and layers.1")
    F, Cin = w1.shape
    E = w2.shape[0]
    if x.shape[-1] != Cin or w2.shape[1] != F:
        raise ValueError(f"ffn_block: x [..., {x.shape[-1]}] against layers.0.0.weight {tuple(w1.shape)}, layers.1.weight {tuple(w2.shape)}")
    for i, width in ((0, Cin), (1, Cin), (3, F), (5, E), (7, E), (8, E), (9, E)):
        if params[i] is not None and tuple(params[i].shape) != (width,):
            raise ValueError(f"ffn_block: parameter {i} of the table has shape {tuple(params[i].shape)}, not ({width},)")
    if params[6] is not None and tuple(params[6].shape) != (E, Cin):
        raise ValueError(f"ffn_block: identity_fc.weight {tuple(params[6].shape)} is not ({E}, {Cin})")
    lead = x.shape[:-1]
    xa = _lib.aligned(x).reshape(-1, Cin)
    res = None
    if residual is not None:
        if tuple(residual.shape) != (*lead, E):
            raise ValueError(f"ffn_block: residual {tuple(residual.shape)} is not {(*lead, E)}")
        res = _lib.aligned(residual).reshape(-1, E)
    return xa, res, lead, Cin, F, E


def _launch(x, params, residual):
    """The library call on the 10-entry parameter list; the callers have settled autograd."""
    xa, res, lead, Cin, F, E = _shape(x, params, residual)
    table, held = _lib.param_table(params, _lib.GF_FFN_PARAMS)
    out = torch.empty(xa.shape[0], E, dtype=f32, device=xa.device)
    _lib.call("gf_ffn_forward", xa.device, xa.shape[0], Cin, F, E, xa, table, res, out)
    return out.view(*lead, E)


def ffn_block(x, ffn, norm=None, residual=None):
    """``out [..., 128] = norm(ffn(x) + residual)`` in one launch, on any leading shape: ``AsymmetricFFN.forward(x)`` (its
    ``pre_norm`` and ``identity_fc`` where the module has them), then ``+ residual [..., 128]`` and the ``nn.LayerNorm(128)``
    ``norm`` where given -- the encoder's ``"ffn", "norm"`` and ``"identity", "ffn", "add", "norm"``.  ``ffn``: a module with the
    reference's submodule names, or a mapping with its state_dict keys (``pre_norm.*``, ``layers.0.0.*``, ``layers.1.*``,
    ``identity_fc.*``); ``norm``: an ``nn.LayerNorm``, a ``(weight, bias)`` pair or ``None``.  Dropout is not applied (eval
    semantics); the parameters are read in place at every call.  Forward only: inputs that need autograd are refused."""
    params = _param_list(ffn, norm)
    _lib.refuse_autograd("ffn_block", [x, residual, *params], "(the AsymmetricFFN module routes training to its torch layers)")
    return _launch(x, params, residual)


def train_sizes(n, cin):
    """``(saved_bytes, workspace_bytes)`` of the training step on ``n`` rows of width ``cin`` (``gf_ffn_train_sizes``)."""
    return _lib.train_sizes("gf_ffn_train_sizes", n, cin)


def _keep_mask(keep, p, shape, device, what):
    """``(mask, scale)`` of one dropout: the caller's keep mask as it is where it has one byte per entry (bool, uint8), any
    other dtype as ``!= 0``; without one and with ``p > 0``, a mask drawn on the current generator straight into uint8 (no
    float32 transient, capturable); ``(None, 1.0)`` when there is no dropout.  The scale is ``1 / (1 - p)``."""
    if not 0.0 <= p < 1.0:
        raise ValueError(f"ffn_block_autograd: {what} = {p} is not in [0, 1)")
    if keep is None:
        if p == 0.0:
            return None, 1.0
        keep = torch.empty(shape, dtype=torch.uint8, device=device).bernoulli_(1.0 - p)
    else:
        _lib.require_gpu(keep)
        if tuple(keep.shape) != tuple(shape):
            raise ValueError(f"ffn_block_autograd: the mask of {what} has shape {tuple(keep.shape)}, not {tuple(shape)}")
        keep = keep.detach()
        if keep.dtype == torch.bool:
            keep = keep.contiguous().view(torch.uint8)
        elif keep.dtype != torch.uint8:
            keep = (keep != 0).to(torch.uint8)
        keep = keep.contiguous()
    return keep, 1.0 / (1.0 - p)


class FFNBlockFunction(torch.autograd.Function):
    """``out = FFNBlockFunction.apply(x, residual, keep_hidden, scale_hidden, keep_out, scale_out, *params)`` on the 10-entry
    parameter list (``None`` for an absent part) and the two keep masks (uint8, ``None``: no dropout there):
    ``gf_ffn_forward_train`` keeps the row before the post norm and the norms' statistics, ``gf_ffn_backward`` returns the
    gradients of ``x``, the residual and every parameter that requires one.  Once-differentiable."""

    @staticmethod
    def forward(ctx, x, residual, keep_hidden, scale_hidden, keep_out, scale_out, *params):
        xa, res, lead, Cin, F, E = _shape(x, params, residual)
        slots, table, held = _lib.ParamSlots.pack(params, _lib.GF_FFN_PARAMS)
        n = xa.shape[0]
        saved_bytes, _ = train_sizes(n, Cin)
        saved = torch.empty(saved_bytes, dtype=torch.uint8, device=xa.device)
        out = torch.empty(n, E, dtype=f32, device=xa.device)
        _lib.call("gf_ffn_forward_train", xa.device, n, Cin, F, E, xa, table, res, keep_hidden, scale_hidden, keep_out, scale_out,
                  out, saved, saved_bytes)
        ctx.save_for_backward(xa, saved, keep_hidden, keep_out, *held)
        ctx.shape = (lead, Cin, F, E, scale_hidden, scale_out, x.dtype, None if residual is None else residual.dtype, slots)
        return out.view(*lead, E)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        xa, saved, keep_hidden, keep_out, *held = ctx.saved_tensors
        lead, Cin, F, E, scale_hidden, scale_out, x_dtype, res_dtype, slots = ctx.shape
        n = xa.shape[0]
        params, table = slots.unpack(held)
        grads, gtable = slots.grad_buffers(params, [True] * len(params))     # every present parameter
        _, work_bytes = train_sizes(n, Cin)
        work = torch.empty(work_bytes, dtype=torch.uint8, device=xa.device)
        grad_x = torch.empty(n, Cin, dtype=f32, device=xa.device)
        need = ctx.needs_input_grad
        grad_res = torch.empty(n, E, dtype=f32, device=xa.device) if res_dtype is not None and need[1] else None
        go = _lib.aligned(grad_out).reshape(n, E)
        _lib.call("gf_ffn_backward", xa.device, n, Cin, F, E, xa, table, keep_hidden, scale_hidden, keep_out, scale_out, saved, go,
                  grad_x, grad_res, gtable, work, work_bytes)
        return (grad_x.view(*lead, Cin).to(x_dtype) if need[0] else None,
                None if grad_res is None else grad_res.view(*lead, E).to(res_dtype), None, None, None, None,
                *slots.returned(grads, need[6:]))


def ffn_block_autograd(x, ffn, norm=None, residual=None, p_hidden=0.0, p_out=0.0, keep_hidden=None, keep_out=None):
    """``ffn_block`` with the module's two dropouts and a native backward: ``out [..., 128]`` carries the graph of
    ``FFNBlockFunction``, so ``x``, the residual and every parameter that requires grad receive their gradients (the others
    ``None``).  ``p_hidden`` / ``p_out``: the probabilities of the dropout behind the ReLU (``layers.0.2``) and behind
    ``layers.1`` (``layers.2``); the kept entries are scaled by ``1 / (1 - p)``.  ``keep_hidden [..., 512]`` / ``keep_out
    [..., 128]``: the keep masks (nonzero = keep), used as they are where bool or uint8; without one and with ``p > 0`` the mask
    is drawn here, as uint8, on the current generator.  Without any dropout and with nothing that needs autograd (or under
    ``torch.no_grad()``) it is ``ffn_block``."""
    params = _param_list(ffn, norm)
    lead = tuple(x.shape[:-1])
    keep_hidden, scale_hidden = _keep_mask(keep_hidden, p_hidden, (*lead, F_NATIVE), x.device, "p_hidden")
    keep_out, scale_out = _keep_mask(keep_out, p_out, (*lead, E_NATIVE), x.device, "p_out")
    if keep_hidden is None and keep_out is None and not _lib.needs_grad([x, residual, *params]):
        return _launch(x, params, residual)
    return FFNBlockFunction.apply(x, residual, keep_hidden, scale_hidden, keep_out, scale_out, *params)


def _build_norm(cfg, width):
    cfg = dict(cfg)
    kind = cfg.pop("type", None)
    if kind != "LN":
        raise NotImplementedError(f"AsymmetricFFN: pre_norm of type {kind!r} (only 'LN' is built here)")
    cfg.pop("requires_grad", None)
    return nn.LayerNorm(width, **cfg)


def _build_activation(cfg):
    cfg = dict(cfg)
    kind = cfg.pop("type", None)
    if kind == "ReLU":
        return nn.ReLU(**cfg)
    if kind == "GELU":
        return nn.GELU(**cfg)
    raise NotImplementedError(f"AsymmetricFFN: act_cfg of type {kind!r} (only 'ReLU' and 'GELU' are built here)")


def _build_dropout(cfg):
    cfg = dict(cfg)
    kind = cfg.pop("type", None)
    if kind != "Dropout":
        raise NotImplementedError(f"AsymmetricFFN: dropout_layer of type {kind!r} (only 'Dropout' is built here)")
    return nn.Dropout(p=cfg.pop("drop_prob", 0.5), **cfg)


class AsymmetricFFN(nn.Module):
    """Same constructor keys and defaults, attributes, submodule names, ``state_dict`` keys and ``forward(x, identity=None)`` as
    the reference class (ffn_module.py:8-75), so its checkpoints load with ``strict=True``; built without mmcv
    (``pre_norm=dict(type="LN")``, ``act_cfg`` of type ``ReLU`` or ``GELU``, ``dropout_layer`` ``None`` or
    ``dict(type="Dropout", drop_prob=p)``; anything else raises ``NotImplementedError``).  The reference's quirk is kept:
    ``identity_fc`` is ``Linear(self.in_channels, embed_dims)`` whenever ``feedforward_channels != embed_dims`` and
    ``Identity`` otherwise (:60-64).

    The native op runs when ``x`` is an fp32 GPU tensor, ``identity is None``, ``num_fcs == 2`` with ReLU, ``embed_dims == 128``,
    ``feedforward_channels == 512``, the input width is 128 or 256, nothing needs autograd, and the module is in eval mode or
    every dropout probability is 0.  Everything else runs ``forward_torch``, the reference's composition on the module's own
    layers.

    ``native_training`` is an attribute, not a constructor key (the constructor stays the reference's), off by default and not
    part of the ``state_dict``: set ``module.native_training = True`` and, under the same conditions, a call that needs autograd
    or has an active ``ffn_drop`` runs ``FFNBlockFunction`` (the masks drawn with ``layers[0][2].p`` and ``layers[2].p``)
    instead of the torch layers.  An active ``dropout_layer`` still goes to torch."""

    native_training = False

    def __init__(self, in_channels=None, pre_norm=None, embed_dims=256, feedforward_channels=1024, num_fcs=2,
                 act_cfg=dict(type="ReLU", inplace=True), ffn_drop=0.0, dropout_layer=None, add_identity=True, init_cfg=None,
                 **kwargs):
        super().__init__()
        assert num_fcs >= 2, f"num_fcs should be no less than 2. got {num_fcs}."
        self.init_cfg = init_cfg
        self.in_channels = in_channels
        self.pre_norm = pre_norm
        self.embed_dims = embed_dims
        self.feedforward_channels = feedforward_channels
        self.num_fcs = num_fcs
        self.act_cfg = act_cfg
        self.activate = _build_activation(act_cfg)
        layers = []
        if in_channels is None:
            in_channels = embed_dims
        if pre_norm is not None:
            self.pre_norm = _build_norm(pre_norm, in_channels)
        for _ in range(num_fcs - 1):
            layers.append(nn.Sequential(nn.Linear(in_channels, feedforward_channels), self.activate, nn.Dropout(ffn_drop)))
            in_channels = feedforward_channels
        layers.append(nn.Linear(feedforward_channels, embed_dims))
        layers.append(nn.Dropout(ffn_drop))
        self.layers = nn.Sequential(*layers)
        self.dropout_layer = _build_dropout(dropout_layer) if dropout_layer else nn.Identity()
        self.add_identity = add_identity
        if self.add_identity:
            # (the reference's local in_channels is feedforward_channels by now)
            self.identity_fc = nn.Identity() if in_channels == embed_dims else nn.Linear(self.in_channels, embed_dims)

    def _dropout_active(self):
        return self.training and any(isinstance(m, nn.Dropout) and m.p > 0 for m in self.modules())

    def _native(self, x, identity):
        if identity is not None or not (x.is_cuda and x.dtype == f32) or self.num_fcs != 2 or not isinstance(self.activate, nn.ReLU):
            return False
        first = self.layers[0][0]
        if self.embed_dims != E_NATIVE or self.feedforward_channels != F_NATIVE or first.in_features not in CIN_NATIVE:
            return False
        if not (first.weight.is_cuda and first.weight.dtype == f32):
            return False
        return _lib.norm_native(self.pre_norm)     # (the kernel's pre norm is the post norm's LayerNorm: affine, eps 1e-5)

    def forward(self, x, identity=None):
        if self._native(x, identity):
            params = _param_list(self, None)
            if not self._dropout_active():
                if not _lib.needs_grad([x, *params]):
                    return _launch(x, params, None)
                if self.native_training:
                    return FFNBlockFunction.apply(x, None, None, 1.0, None, 1.0, *params)
            elif self.native_training and not (isinstance(self.dropout_layer, nn.Dropout) and self.dropout_layer.p > 0):
                p_hidden, p_out = self.layers[0][2].p, self.layers[2].p
                if p_hidden < 1.0 and p_out < 1.0:
                    return ffn_block_autograd(x, self, p_hidden=p_hidden, p_out=p_out)
        return self.forward_torch(x, identity)

    def forward_torch(self, x, identity=None):
        """The reference's composition (:66-75) on the module's torch layers."""
        if self.pre_norm is not None:
            x = self.pre_norm(x)
        out = self.layers(x)
        if not self.add_identity:
            return self.dropout_layer(out)
        if identity is None:
            identity = x
        identity = self.identity_fc(identity)
        return identity + self.dropout_layer(out)
