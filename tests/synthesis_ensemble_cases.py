"""Shapes and builders shared by tests/test_gpu_synthesis_ensemble.py and tests/test_synthesis_ensemble_host.py (no test in here).

Shapes are (B, C, T, out_dim, conv_channels, lstm_hidden, label_dim, L):
  S1  two time tiles; T/2 = 35 is odd, so the second pool drops a sample; ldf 576 != F + H 573 and ldd 8 != 7: padded fc.1
      weight, slab copies, the ``_colsum`` path; L = 1: zero W_hh gradient; generic conv / LSTM loops
  S2  direct-write paths, register-resident LSTM (H = 64), masked W_hh rows
  S3  128-row GEMM tiles, B L - 1 = 324
"""
import torch

S1 = (3, 5, 70, 7, 33, 12, 1, 1)
S2 = (5, 4, 64, 80, 16, 64, 2, 5)
S3 = (65, 4, 64, 80, 16, 64, 2, 5)
SHAPES = {"S1": S1, "S2": S2, "S3": S3}
M = 3
SEEDS = (11, 23, 37)                 # the members' torch seeds
SENTINEL = -12345.0


def r4(n):
    return (n + 3) // 4 * 4


def dims(cfg):
    B, C, T, D, CC, H, ld, L = cfg
    T1, T2 = T // 2, T // 2 // 2
    F = CC * T2
    return dict(B=B, C=C, T=T, D=D, CC=CC, H=H, ld=ld, L=L, T1=T1, T2=T2, F=F, ldf=r4(F + H), ldd=r4(D), hid=512)


def lite_models(cfg, seeds=SEEDS, dropout=0.3):
    """One SynthesisLite per seed (distinct initial weights), on the CPU."""
    from decode_tonal_langauge_amd.models.synthesis_models import SynthesisLite
    B, C, T, D, CC, H, ld, L = cfg
    models = []
    for s in seeds:
        torch.manual_seed(s)
        models.append(SynthesisLite(D, C, T, label_dim=ld, conv_channels=CC, lstm_hidden=H, dropout=dropout))
    return models


def step_batches(cfg, members, steps, seed=5):
    """[step][member] -> (x (B, C, T), labels (B, label_dim, L), targets (B, D)): fixed batches and given labels."""
    B, C, T, D, CC, H, ld, L = cfg
    g = torch.Generator().manual_seed(seed)
    return [[(torch.randn(B, C, T, generator=g), torch.randn(B, ld, L, generator=g), 10 * torch.randn(B, D, generator=g))
             for _ in range(members)] for _ in range(steps)]


def classifiers(T, n_chan=8):
    """A tone (4 classes) and a syllable (2 classes) logistic classifier with fixed weights."""
    from decode_tonal_langauge_amd.models.simple_classifiers import LogisticRegressionClassifier
    torch.manual_seed(3)
    return LogisticRegressionClassifier(n_chan * T, 4), LogisticRegressionClassifier(n_chan * T, 2)
