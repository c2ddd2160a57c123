"""CPU reference of the ``CNNClassifier`` training tests - TEST INFRASTRUCTURE (no test functions).

``forward`` restates ``CNNClassifier.forward`` + ``F.cross_entropy`` on the model's sigmoid outputs (reference
models/deep_classifiers.py:62-99 under models/classifier_trainer.py:72-89) functionally, in the dtype of the parameters it is
handed, with its DISCRETE branches as optional inputs:
  pooled stage    sel = where(odd, z_odd, z_even), out = where(pos, sel, slope * sel)
  un-pooled / fc1 out = where(pos, z, slope * z)
  dropout         out = h * keep / (1 - p) for a given keep mask.
Autograd through ``where`` with fixed masks routes the gradients exactly as the HIP backward does with its arg-max and sign
planes; without planes the function decides for itself (torch's rules: the first maximum of a pool pair, LeakyReLU' = slope
at exactly 0) and reports those decisions and how far each was from flipping - the pattern of
``oracle.synthesis_oracle.cnn_forward(decisions=, own=, margins=)``.  Two correct fp32 implementations take a handful of
near-tie branches differently and each flip moves a conv gradient by O(1) of one element, so gradient comparisons hand HIP's
planes over - after ``tests.branch_planes.check_flips`` held them to the reference's own.

``hip_planes`` / ``hip_keep_mask`` read the branches a ``CnnClassifierTrainEngine`` took, in torch's layout (B, ch, t, C)."""
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.branch_planes import bit_plane

SHAPES = [((3, 2, 150, 2), 0), ((2, 3, 200, 5), 1), ((5, 4, 151, 4), 2), ((65, 2, 150, 3), 3)]     # (B, C, T, n), seed


def build(shape, seed: int, dropout: float = 0.5):
    """(model, x, y): the model built after ``torch.manual_seed(seed)``, the input drawn with ``randn`` behind it."""
    from decode_tonal_langauge_amd.models.deep_classifiers import CNNClassifier
    B, Cn, T, n = shape
    torch.manual_seed(seed)
    model = CNNClassifier(Cn, T, n, dropout_rate=dropout)
    x = torch.randn(B, Cn, T)
    y = torch.randint(0, n, (B,))
    return model, x, y


def stages(model) -> List[Tuple[str, bool]]:
    """[(parameter prefix of the conv, pooled)] of ``model.feature_extractor``"""
    out = []
    for i, m in enumerate(model.feature_extractor):
        if isinstance(m, nn.Conv2d):
            out.append([f"feature_extractor.{i}", False])
        elif isinstance(m, nn.MaxPool2d):
            out[-1][1] = True
    return [tuple(s) for s in out]


def leaves(model, dtype) -> Dict[str, torch.Tensor]:
    return {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in model.named_parameters()}


def forward(model, p: Dict[str, torch.Tensor], x: torch.Tensor, planes: Optional[dict] = None,
            keep: Optional[torch.Tensor] = None, own: Optional[dict] = None, margins: Optional[dict] = None) -> torch.Tensor:
    """Sigmoid scores (B, n).  ``planes``: {"conv<i>.odd" / "conv<i>.pos" (i = 1..6), "fc1.pos"} bool tensors; layers without
    an entry decide for themselves.  ``keep``: bool (B, ch, t, C) dropout keep mask (None: no dropout).  ``own`` / ``margins``:
    dicts that receive this pass's own decisions and |z_odd - z_even|, |sel| and "<layer>.scale" = max|z|."""
    planes = planes or {}
    slope = float(model._hip_cfg[2])
    p_drop = float(model.feature_extractor[-1].p)
    dtype = next(iter(p.values())).dtype

    def note(key, kind, decision, margin):
        if own is not None:
            own[f"{key}.{kind}"] = decision.detach()
        if margins is not None:
            margins[f"{key}.{kind}"] = margin.detach()

    def act(key, z):
        pos = z.detach() > 0
        note(key, "pos", pos, z.abs())
        if margins is not None:
            margins.setdefault(f"{key}.scale", float(z.detach().abs().max()))
        pos = planes.get(f"{key}.pos", pos)
        return torch.where(pos, z, slope * z)

    h = x.to(dtype).unsqueeze(1).permute(0, 1, 3, 2)                       # (B, 1, T, C)
    for i, (name, pool) in enumerate(stages(model), start=1):
        key = f"conv{i}"
        z = F.conv2d(h, p[name + ".weight"], p[name + ".bias"])
        if margins is not None:
            margins[f"{key}.scale"] = float(z.detach().abs().max())
        if pool:
            t2 = z.shape[2] // 2
            ze, zo = z[:, :, 0:2 * t2:2], z[:, :, 1:2 * t2:2]
            odd = zo.detach() > ze.detach()                                  # max_pool2d keeps the FIRST maximum of a tie
            note(key, "odd", odd, (zo - ze).abs())
            z = torch.where(planes.get(f"{key}.odd", odd), zo, ze)
        h = act(key, z)
    if keep is not None:
        h = h * keep.to(dtype) / (1.0 - p_drop)
    a1 = act("fc1", h.flatten(1) @ p["classifier.1.weight"].t() + p["classifier.1.bias"])
    return torch.sigmoid(a1 @ p["classifier.3.weight"].t() + p["classifier.3.bias"])


def loss_and_grads(model, p, x, y, **kw):
    """(scores, mean CE loss on the scores, {name: gradient}) of ``forward``."""
    s = forward(model, p, x, **kw)
    loss = F.cross_entropy(s, y.long())
    g = torch.autograd.grad(loss, list(p.values()))
    return s.detach(), loss.detach(), dict(zip(p.keys(), g))


def stock_loss_and_grads(model, x, y, dtype):
    """The same from the stock module (autograd through ``model.forward`` in eval mode, i.e. without dropout)."""
    import copy
    m = copy.deepcopy(model).cpu().to(dtype).eval()
    s = m(x.to(dtype))
    loss = F.cross_entropy(s, y.long())
    loss.backward()
    return s.detach(), loss.detach(), {k: v.grad.detach() for k, v in m.named_parameters()}


# ---------------------------------------------------------------------------------------------- readers of the engine's state
def hip_planes(eng, B: int) -> dict:
    """Every discrete branch the engine's backward takes after a forward pass at batch ``B``: arg-max and "pooled output > 0"
    planes of the pooled stages, the sign of the stored rows of an un-pooled stage, fc1's sign off the stored a1."""
    Cn, S = eng.C, B * eng.C
    dec = {"conv1.odd": bit_plane(eng.bits[1], S, eng.tp1, eng.tout1, B, Cn),
           "conv1.pos": bit_plane(eng.sbits[1], S, eng.tp1, eng.tout1, B, Cn)}
    for st in eng.stages:
        key = f"conv{st.idx}"
        if st.pool:
            dec[key + ".odd"] = bit_plane(eng.bits[st.idx], S, st.tp_out, st.tout, B, Cn)
            dec[key + ".pos"] = bit_plane(eng.sbits[st.idx], S, st.tp_out, st.tout, B, Cn)
        else:
            rows = eng.P[st.idx]
            dec[key + ".pos"] = (rows.view(B, Cn, st.tp_out, rows.shape[1])[:, :, :st.tout, :st.cout] > 0) \
                .permute(0, 3, 2, 1).contiguous().cpu()
    dec["fc1.pos"] = (eng._heads[B].a1 > 0).cpu()
    return dec


def hip_keep_mask(eng, B: int) -> Optional[torch.Tensor]:
    """The dropout keep mask of the engine's last forward pass (None: none applied), bool (B, ch, lat, C): ``tl_dropout_scale``
    with the step's seed over ones in the shape of the feature rows, re-indexed as the features are."""
    from decode_tonal_langauge_amd import _lib
    if not eng.last_seed:
        return None
    ones = torch.ones(B * eng.C * eng.tp_last, eng.ld_last, device=eng.device)
    _lib.check(eng.lib.tl_dropout_scale(ones.data_ptr(), ones.numel(), eng.p_drop, eng.last_seed,
                                        torch.cuda.current_stream().cuda_stream), "tl_dropout_scale")
    m = ones.view(B, eng.C, eng.tp_last, eng.ld_last)[:, :, :eng.lat, :eng.c_last] != 0
    return m.permute(0, 3, 2, 1).contiguous().cpu()
