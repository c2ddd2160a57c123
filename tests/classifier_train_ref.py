"""CPU references of the classifier-training tests - TEST INFRASTRUCTURE.

``parent_fit`` is the loop ``ClassifierTrainer`` ran before it gained ``fused`` (autograd, ``torch.optim.NAdam`` with the two
decay groups, per-batch host reads), kept here unchanged: in float32 it pins the ``fused=False`` path bit for bit, in float64
it is the reference of the fused path.  ``rel_l2`` is the deviation every numeric comparison uses; ``yardstick`` of a quantity
is ``rel_l2`` of the float32 CPU evaluation against the float64 one, and a bound is 10 yardsticks."""
import copy
from typing import Dict, List

import torch
import torch.nn as nn
from torch.optim import NAdam

FACTOR = 10.0


def rel_l2(got, ref) -> float:
    got = torch.as_tensor(got).detach().double().cpu().reshape(-1)
    ref = torch.as_tensor(ref).detach().double().cpu().reshape(-1)
    return float((got - ref).norm() / ref.norm().clamp(min=1e-300))


def planted(n: int, n_cls: int = 4, channels: int = 16, length: int = 100, seed: int = 0):
    """N(0,1) windows with class k lifting its own group of channels by 0.5 (data_loading/synthetic.py)."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, n_cls, (n,), generator=g)
    x = torch.randn(n, channels, length, generator=g)
    grp = channels // n_cls
    for k in range(n_cls):
        x[y == k, k * grp:(k + 1) * grp] += 0.5
    return x, y.float()


def batches(x, y, batch: int):
    return [(x[i:i + batch], y[i:i + batch]) for i in range(0, len(y), batch)]


def nadam_two_groups(model, lr: float, weight_decay: float, decay_biases: bool = False) -> NAdam:
    decay = [p for p in model.parameters() if p.ndim >= 2]
    rest = [p for p in model.parameters() if p.ndim < 2]
    return NAdam([{"params": decay, "weight_decay": weight_decay},
                  {"params": rest, "weight_decay": weight_decay if decay_biases else 0.0}], lr=lr)


def _confusion(true, pred, n):
    return torch.bincount(true.long() * n + pred.long(), minlength=n * n).reshape(n, n)


def parent_run_epoch(model, optimizer, loader, train: bool) -> Dict[str, float]:
    from decode_tonal_langauge_amd.models.classifier_trainer import macro_scores
    criterion = nn.CrossEntropyLoss()
    n_cls = model.n_classes
    loss_sum, n_seen = 0.0, 0
    cm = torch.zeros(n_cls, n_cls, dtype=torch.long)
    model.train(train)
    for x, y in loader:
        y = y.long()
        with torch.set_grad_enabled(train):
            logits = model(x)
            loss = criterion(logits, y)
        if train:
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
        loss_sum += float(loss.detach()) * len(y)
        n_seen += len(y)
        cm += _confusion(y.cpu(), logits.detach().argmax(1).cpu(), n_cls)
    return {"loss": loss_sum / max(n_seen, 1), "accuracy": macro_scores(cm)["accuracy"]}


def parent_fit(model, lr: float, weight_decay: float, train_loader, val_loader, epochs: int) -> List[Dict[str, float]]:
    opt = nadam_two_groups(model, lr, weight_decay)
    history, step = [], 0
    for epoch in range(epochs):
        tr = parent_run_epoch(model, opt, train_loader, True)
        step += len(train_loader)
        va = parent_run_epoch(model, opt, val_loader, False)
        wn = float(sum(float(p.detach().norm(2)) ** 2 for p in model.parameters() if p.requires_grad) ** 0.5)
        history.append({"epoch": epoch, "step": step - 1, "train/loss_epoch": tr["loss"], "train/accuracy": tr["accuracy"],
                        "val/loss": va["loss"], "val/accuracy": va["accuracy"], "train/weight_norm": wn})
    return history


def as_double(model, data):
    """(float64 copy of ``model`` on the CPU, ``data`` batches with float64 inputs)."""
    return copy.deepcopy(model).cpu().double(), [(x.double(), y) for x, y in data]


def updates_after(model, data, lr: float, weight_decay: float, decay_biases: bool = False) -> Dict[str, torch.Tensor]:
    """theta_after - theta_before per parameter name after one NAdam step per batch of ``data`` (autograd, CPU, the model's
    dtype); ``model`` is left untouched."""
    m = copy.deepcopy(model)
    before = {k: v.detach().clone() for k, v in m.named_parameters()}
    opt = nadam_two_groups(m, lr, weight_decay, decay_biases)
    for x, y in data:
        opt.zero_grad()
        nn.functional.cross_entropy(m(x.reshape(len(y), -1)), y.long()).backward()
        opt.step()
    return {k: v.detach() - before[k] for k, v in m.named_parameters()}


def gradients(model, x, y) -> Dict[str, torch.Tensor]:
    m = copy.deepcopy(model)
    nn.functional.cross_entropy(m(x.reshape(len(y), -1)), y.long()).backward()
    return {k: v.grad.detach() for k, v in m.named_parameters()}
