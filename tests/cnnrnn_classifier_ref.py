"""CPU reference of the ``CNNRNNClassifier`` training tests - TEST INFRASTRUCTURE (no test functions).

``forward`` restates ``CNNRNNClassifier.forward`` + ``F.cross_entropy`` on the model's sigmoid outputs (reference
models/deep_classifiers.py:158-343 under models/classifier_trainer.py:72-89) functionally, in the dtype of the leaves it is
handed, with its DISCRETE branches as optional inputs:
  block1 / block2   sel = where(odd, z_odd, z_even), out = where(pos, sel, slope * sel)       (conv (7,1) + LeakyReLU + pool (2,1))
  conv3a / conv3b   out = where(pos, z, slope * z)
  pool3             out = the row ``arg`` (0..2) of every triple of conv3b's activation
  dropout           out = h * keep / (1 - p) for a given keep mask.
Autograd through ``where`` / ``gather`` with fixed planes routes the gradients exactly as the HIP backward does; without planes
the function decides for itself by torch's rules (the first maximum of a pool window, LeakyReLU' = slope at exactly 0) and
reports its decisions and how far each was from flipping (``own=`` / ``margins=``, with ``<layer>.scale`` = max |z|), the pattern
of ``tests/cnn_classifier_ref.py``.  ``pool3.arg``'s margin is the gap between the two largest values of the triple.

``hip_planes`` / ``hip_keep_mask`` read the branches a ``CnnRnnClassifierTrainEngine`` took, in torch's layout."""
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from tests.branch_planes import bit_plane

#: (B, C, T, lstm_dim, n_classes), seed
SHAPES = [((3, 2, 60, 60, 2), 0), ((5, 3, 50, 100, 4), 1), ((2, 5, 44, 132, 3), 2), ((33, 2, 48, 48, 3), 3)]
PLANES = ("block1.odd", "block1.pos", "block2.odd", "block2.pos", "conv3a.pos", "conv3b.pos", "pool3.arg")


def build(shape, seed: int, dropout: float = 0.5):
    """(model, x, y): the model built after ``torch.manual_seed(seed)``, the input drawn with ``randn`` behind it."""
    from decode_tonal_langauge_amd.models.deep_classifiers import CNNRNNClassifier
    B, Cn, T, lstm_dim, n = shape
    torch.manual_seed(seed)
    model = CNNRNNClassifier(Cn, T, n, lstm_dim=lstm_dim, dropout=dropout)
    x = torch.randn(B, Cn, T)
    y = torch.randint(0, n, (B,))
    return model, x, y


def leaves(model, dtype) -> Dict[str, torch.Tensor]:
    return {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in model.named_parameters()}


def lstm_last(x: torch.Tensor, w_ih, w_hh, b_ih, b_hh) -> torch.Tensor:
    """h_T of a one-layer LSTM with zero initial state over x (B, T, in); torch's gate order i, f, g, o."""
    B, H = x.shape[0], w_hh.shape[1]
    h = x.new_zeros(B, H)
    c = x.new_zeros(B, H)
    xp = x @ w_ih.t() + (b_ih + b_hh)
    for t in range(x.shape[1]):
        i, f, g, o = (xp[:, t] + h @ w_hh.t()).chunk(4, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
    return h


def forward(model, p: Dict[str, torch.Tensor], x: torch.Tensor, planes: Optional[dict] = None,
            keep: Optional[torch.Tensor] = None, own: Optional[dict] = None, margins: Optional[dict] = None) -> torch.Tensor:
    """Sigmoid scores (B, n).  ``planes``: entries of ``PLANES`` (bool, ``pool3.arg`` int64) in torch's activation layout; layers
    without an entry decide for themselves.  ``keep``: bool (B, 256, t', W) dropout keep mask (None: no dropout)."""
    planes = planes or {}
    slope = float(model.conv_pool_block1[1].negative_slope)
    p_drop = float(model.conv_block3[5].p)
    dtype = next(iter(p.values())).dtype
    B, _, T = x.shape

    def note(key, kind, decision, margin):
        if own is not None:
            own[f"{key}.{kind}"] = decision.detach()
        if margins is not None:
            margins[f"{key}.{kind}"] = margin.detach()

    def scale(key, z):
        if margins is not None:
            margins[f"{key}.scale"] = float(z.detach().abs().max())

    def act(key, z):
        pos = z.detach() > 0
        note(key, "pos", pos, z.abs())
        return torch.where(planes.get(f"{key}.pos", pos), z, slope * z)

    def block(key, name, h):
        z = F.conv2d(h, p[name + ".weight"], p[name + ".bias"])
        scale(key, z)
        t2 = z.shape[2] // 2
        ze, zo = z[:, :, 0:2 * t2:2], z[:, :, 1:2 * t2:2]
        odd = zo.detach() > ze.detach()                                  # max_pool2d keeps the FIRST maximum of a tie
        note(key, "odd", odd, (zo - ze).abs())
        return act(key, torch.where(planes.get(f"{key}.odd", odd), zo, ze))

    def conv(key, name, h):
        z = F.conv2d(h, p[name + ".weight"], p[name + ".bias"])
        scale(key, z)
        return act(key, z)

    xt = x.to(dtype).permute(0, 2, 1)                                      # (B, T, C)
    lw = lambda n: (p[n + ".weight_ih_l0"], p[n + ".weight_hh_l0"], p[n + ".bias_ih_l0"], p[n + ".bias_hh_l0"])
    h1 = lstm_last(xt, *lw("lstm1"))
    a = block("block1", "conv_pool_block1.0", xt.unsqueeze(1))             # (B, 1024, t1, C)
    b = block("block2", "conv_pool_block2.0", h1.reshape(B, 1, T, -1))     # (B, 1024, t1, w1)
    f = conv("conv3a", "conv_block3.0", torch.cat((b, a), dim=3))
    f = conv("conv3b", "conv_block3.2", f)                                 # (B, 256, tb, W)
    tq = f.shape[2] // 3
    tri = f[:, :, :3 * tq].reshape(B, f.shape[1], tq, 3, f.shape[3])
    arg = tri.detach().argmax(dim=3)                                        # (the first maximum: torch's rule on equal values)
    top = tri.detach().topk(2, dim=3).values
    note("pool3", "arg", arg, top[:, :, :, 0] - top[:, :, :, 1])
    if margins is not None:
        margins["pool3.scale"] = float(f.detach().abs().max())
    arg = planes.get("pool3.arg", arg).long()
    f = tri.gather(3, arg.unsqueeze(3)).squeeze(3)                          # (B, 256, t', W)
    if keep is not None:
        f = f * keep.to(dtype) / (1.0 - p_drop)
    f = f.contiguous().view(B, tq, -1)                                      # raw re-interpretation, as the reference (:315)
    h2 = lstm_last(f, *lw("lstm2"))
    return torch.sigmoid(h2 @ p["output.weight"].t() + p["output.bias"])


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
def _cat_width(eng, B: int, per_seq: torch.Tensor) -> torch.Tensor:
    """(B * W, ...) in the engine's branch-major sequence order -> (B, W, ...) in ``torch.cat((x1, x), dim=3)`` order."""
    nb = B * eng.w1
    return torch.cat((per_seq[:nb].reshape(B, eng.w1, *per_seq.shape[1:]), per_seq[nb:].reshape(B, eng.Cn, *per_seq.shape[1:])),
                     dim=1)


def hip_planes(eng, B: int) -> dict:
    """Every discrete branch the engine's backward takes after a forward pass at batch ``B``, in the layout of ``forward``.
    ``pool3.arg`` is NOT read from the kernel, which stores no plane and recomputes the arg-max in its backward: it is derived
    here from the engine's stored rows with ``argmax``.  On triples without exact ties (random data has none) that is the
    kernel's choice whatever rule either applies; the first-maximum rule itself is pinned by the stand-alone pool test, which
    is exact and plants ties."""
    Tp, t1 = eng.Tp, eng.t1
    nb = B * eng.w1
    dec = {}
    for words, kind in ((eng.bits[1], "odd"), (eng.sbits[1], "pos")):
        # bit_plane: (S * tp, words) -> (B, ch, tout, columns of the branch)
        dec[f"block2.{kind}"] = bit_plane(words[:nb * Tp], nb, Tp, t1, B, eng.w1)
        dec[f"block1.{kind}"] = bit_plane(words[nb * Tp:], B * eng.Cn, Tp, t1, B, eng.Cn)
    S = B * eng.W
    for key, rows, tout in (("conv3a", eng.P[2], eng.ta), ("conv3b", eng.P[3], eng.tb)):
        per_seq = rows[:S * Tp].view(S, Tp, rows.shape[1])[:, :tout] > 0                  # (S, t, ch)
        dec[f"{key}.pos"] = _cat_width(eng, B, per_seq).permute(0, 3, 2, 1).contiguous().cpu()
    tri = eng.P[3].view(S, Tp, -1)[:, :3 * eng.tq].reshape(S, eng.tq, 3, -1)
    arg = tri.argmax(dim=2)                                                                # (S, t', ch): see the docstring
    dec["pool3.arg"] = _cat_width(eng, B, arg).permute(0, 3, 2, 1).contiguous().cpu()
    return dec


def hip_keep_mask(eng, B: int) -> Optional[torch.Tensor]:
    """The dropout keep mask of the engine's last forward pass (None: none applied), bool (B, 256, t', W): ``tl_dropout_scale``
    with the step's seed over ones in the shape of the forward-only engine's (seq, t', 256) buffer, re-indexed."""
    from decode_tonal_langauge_amd import _lib
    if not eng.last_seed:
        return None
    ones = torch.ones(B * eng.W, eng.tq, 256, device=eng.device)
    _lib.check(eng.lib.tl_dropout_scale(ones.data_ptr(), ones.numel(), eng.p_drop, eng.last_seed,
                                        torch.cuda.current_stream().cuda_stream), "tl_dropout_scale")
    return _cat_width(eng, B, ones != 0).permute(0, 3, 2, 1).contiguous().cpu()
