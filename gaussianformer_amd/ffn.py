"""The encoder's feed-forward block: drop-in for ``AsymmetricFFN`` (model/encoder/gaussian_encoder/ffn_module.py:8-75) and the
one-launch form of the ``"ffn", "norm"`` and ``"identity", "ffn", "add", "norm"`` runs of the encoder's ``operation_order``.
torch runs a block as two LayerNorms, three GEMMs, a ReLU and an add around an ``[A, 512]`` hidden tensor;
``gf_ffn_forward`` (include/gf_hip.h) is one launch in which the hidden row never reaches memory.  Forward
only: training, dropout and everything the native op does not cover run the module's own torch layers."""
import ctypes

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
    if norm is None:
        params += [None, None]
    elif isinstance(norm, nn.LayerNorm):
        if norm.eps != 1e-5 or norm.weight is None or norm.bias is None:
            raise ValueError("ffn_block: the post norm must be an affine LayerNorm with eps = 1e-5")
        params += [norm.weight, norm.bias]
    else:
        weight, bias = norm
        params += [weight, bias]
    return params


def _needs_grad(tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _table(params):
    """The library's host table of the 10 pointers, and the tensors it points into: a parameter as it is, or its converted copy
    (another dtype, not contiguous, misaligned), which the caller keeps alive until the launch is queued."""
    table = (ctypes.c_void_p * _lib.GF_FFN_PARAMS)()
    held = []
    for i, p in enumerate(params):
        if p is None:
            continue
        if p.dtype != f32 or not p.is_contiguous() or p.data_ptr() % 16:   # (a module's own parameters: never)
            p = _lib.as_arg(p)
            p = p.clone() if p.data_ptr() % 16 else p
        held.append(p)
        table[i] = p.data_ptr()
    return ctypes.cast(table, ctypes.c_void_p), held


def _aligned(t):
    t = _lib.as_arg(t)
    return t.clone() if t is not None and t.data_ptr() % 16 else t


def _launch(x, params, residual):
    """The library call on the 10-entry parameter list; the callers have settled autograd."""
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
    xa = _aligned(x).reshape(-1, Cin)
    res = None
    if residual is not None:
        if tuple(residual.shape) != (*lead, E):
            raise ValueError(f"ffn_block: residual {tuple(residual.shape)} is not {(*lead, E)}")
        res = _aligned(residual).reshape(-1, E)
    table, held = _table(params)
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
    if _needs_grad([x, residual, *params]):
        raise RuntimeError(
            "ffn_block is a forward without a native backward: call it under torch.no_grad() or with inputs and parameters "
            "that do not require grad (the AsymmetricFFN module routes training to its torch layers)")
    return _launch(x, params, residual)


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
    layers."""

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
        if not (first.weight.is_cuda and first.weight.dtype == f32) or self._dropout_active():
            return False
        if self.pre_norm is not None and (self.pre_norm.eps != 1e-5 or self.pre_norm.weight is None or self.pre_norm.bias is None):
            return False
        return True

    def forward(self, x, identity=None):
        if self._native(x, identity):
            params = _param_list(self, None)
            if not _needs_grad([x, *params]):
                return _launch(x, params, None)
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
