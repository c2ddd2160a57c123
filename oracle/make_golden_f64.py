"""Float64 companion of G4 from the REAL reference (build container only; see make_golden.py for the rules: the reference is
imported read-only, nothing of it is copied, only outputs are stored).

G4 stores the reference's parameters after three fp32 NAdam steps of ``SynthesisModelCNN(80, 16, 200, dropout=0.0)``.  Several
conv biases there have gradients of ~1e-4 that come out of heavily cancelling fp32 sums, and NAdam passes their rounding into
the update: the fp32 update of such a bias moves by up to 3e-3 (relative L2) with the summation order alone - thread count and
vector ISA of the host.  An fp32 comparison against those updates at 1e-3 therefore only holds on a host that rounds like the
one that recorded them.  This script runs the same three steps with the reference evaluated in float64 (same fp32 initial
parameters and inputs, widened) and writes the three-step UPDATE (final - initial) of every parameter, rounded to float32
(6e-8 relative: far below the bound it is checked at), to ``g4f64_cnn_update.npz``: ``upd.<name>`` whole up to SMALL
elements (every bias), else ``upd.<name>@s97`` (every 97th element of the flattened update, as G4 samples).
tests/test_oracle_golden.py compares the oracle's float64 update against it.

Usage:  PYTHONDONTWRITEBYTECODE=1 python oracle/make_golden_f64.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)

from oracle.make_golden import _import_reference  # noqa: E402
from oracle import synthesis_oracle as so  # noqa: E402
from tests import golden_inputs as gi  # noqa: E402

SMALL = 4224          # elements: stored whole up to this size (the largest bias: the LSTM's 4 x 1056 gate rows)


def main():
    rsm = _import_reference()[0]
    torch.set_num_threads(8)
    path = os.path.join(REPO, "tests", "golden", "g4_cnn_train.npz")
    old = np.load(path)
    xs, _t, _s, labs, tg = gi.train_batches(3, 8, 16, 200)
    assert abs(gi.checksum(*xs, *labs, *tg) - float(old["in_checksum"])) < 1e-6 * float(old["in_checksum"])
    torch.manual_seed(0)
    net = rsm.SynthesisModelCNN(80, 16, 200, dropout=0.0).double()
    opt = torch.optim.NAdam(net.parameters(), lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.004)
    crit = torch.nn.L1Loss()
    net.train()
    for s in range(3):                       # the body of the reference's batch loop, as make_golden.py's G4
        opt.zero_grad()
        loss = crit(net(xs[s].double(), labs[s].double()), tg[s].long())
        loss.backward()
        opt.step()
    final = {k: v.detach().numpy() for k, v in net.named_parameters()}
    # the oracle, also in float64, against it
    torch.manual_seed(0)
    p = {k: v.double() for k, v in so.init_cnn_params(80, 16, 200).items()}
    init = {k: v.clone().numpy() for k, v in p.items()}
    st = so.NAdamState(p)
    for s in range(3):
        so.train_step("cnn", p, None, st, xs[s].double(), labs[s].double(), tg[s].double())
    dev = max(gi.update_rel_l2(p[k].numpy(), final[k], init[k]) for k in final)
    out = {"in_checksum": old["in_checksum"]}
    for k, v in final.items():
        upd = (v - init[k]).astype(np.float32)
        if upd.size <= SMALL:
            out["upd." + k] = upd
        else:
            out["upd." + k + "@s97"] = upd.reshape(-1)[::97].copy()
    np.savez_compressed(os.path.join(REPO, "tests", "golden", "g4f64_cnn_update.npz"), **out)
    line = f"g4f64_cnn_update_l2_oracle_vs_reference {dev:.3e}"
    with open(os.path.join(REPO, "tests", "golden", "PINNING.txt"), "a") as f:
        f.write("\n# float64 companion of G4 (oracle/make_golden_f64.py): both sides evaluated in float64\n" + line + "\n")
    print(line)


if __name__ == "__main__":
    main()
