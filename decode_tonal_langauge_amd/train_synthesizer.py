"""Synthesizer training entry point (counterpart of reference train_synthesizer.py).

Two ways in:
 * the reference's argparse CLI (``python -m decode_tonal_langauge_amd.train_synthesizer --sample_path ...``),
   same flags (:29-132);
 * ``run(config)`` for the YAML stage runner (``main.py``): the reference has none - its script is
   not dispatchable by ``main.py`` and fails on import (SURVEY.md section 0 finding 5) - so the
   ``training`` stage can say ``module: decode_tonal_langauge_amd.train_synthesizer`` with
   ``params:`` carrying the same names as the CLI flags.

Inputs (reference :161-201): ``sample_path`` .npz with ``ecog (N,C,T)`` and either ``mel (N, n_mels*frames)``
(pre-computed, what the synthetic generators emit) or ``audio`` (converted by ``utils.audio.audio_to_mel``, the
librosa calls of the reference restated with NumPy / SciPy);
``channel_file`` JSON {active_channels, tone_discriminative, syllable_discriminative};
``config_file`` JSON {mel_kwargs, tone_dynamic_mapping, n_syllables, n_tones[, *_model_kwargs]}.
``--resident`` (YAML: ``resident: true``; off by default) keeps the dataset on the GPU and gathers every batch there.
``--ensemble`` (YAML: ``ensemble: true``; off by default) trains the ``--repeat`` SynthesisLite models side by side in one
pass (``models/synthesis_ensemble_trainer.py``): every member gets the bits the sequential loop gives it.  It implies the
resident dataset and needs ``--synthesis_model_name SynthesisLite``, both classifier checkpoints, a CUDA device, one process.
``--f0_metrics`` (YAML: ``f0_metrics: true``; off by default; needs ``--audio_dir``) tracks F0 on the waveforms written there,
originals and reconstructions in one ``yin_f0_batch`` call, and writes ``f0_metrics.json`` and ``f0_tracks.npz`` beside them.
Output: one CSV row per run with the reference's columns (:369-385).
"""
from __future__ import annotations

import argparse
import json
import os
from argparse import Namespace
from typing import Optional

import numpy as np
import pandas as pd
import torch
from torch.utils.data import TensorDataset

from . import parallel
from .data_loading.dataloaders import split_dataset
from .data_loading.utils import select_non_discriminative_channels
from .models.deep_classifiers import CNNClassifier, CNNRNNClassifier
from .models.simple_classifiers import LogisticRegressionClassifier, ShallowNNClassifier
from .models.synthesis_models import SynthesisLite, SynthesisModelCNN
from .models.synthesis_trainer import SynthesisTrainer
from .utils.utils import set_seeds
from .utils.visualise import plot_training_losses

synthesis_models = ['SynthesisLite', 'SynthesisFull']


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Train an audio synthesizer on ECoG data.")
    p.add_argument('--sample_path', type=str, required=True)
    p.add_argument('--subject_id', type=str, required=True)
    p.add_argument('--result_file', type=str, required=True)
    p.add_argument('--figure_dir', type=str, default=None)
    p.add_argument('--audio_dir', type=str, default=None)
    p.add_argument('--channel_file', type=str, default='channel_selections.json')
    p.add_argument('--config_file', type=str, default='config.json')
    p.add_argument('--model_name', type=str, required=True)
    p.add_argument('--syllable_model_path', type=str, default=None)
    p.add_argument('--tone_model_path', type=str, default=None)
    p.add_argument('--synthesis_model_name', type=str, required=True)
    p.add_argument('--syllable_model_name', type=str, required=True)
    p.add_argument('--tone_model_name', type=str, required=True)
    p.add_argument('--audio_sampling_rate', type=int, default=24414)
    p.add_argument('--seed', type=int, default=42)
    p.add_argument('--repeat', type=int, default=1)
    p.add_argument('--verbose', type=int, default=1)
    p.add_argument('--train_ratio', type=float, default=0.9)
    p.add_argument('--device', type=str, default='cuda:0')
    p.add_argument('--batch_size', type=int, default=8)
    p.add_argument('--epochs', type=int, default=100)
    p.add_argument('--lr', type=float, default=0.0005)
    p.add_argument('--resident', action='store_true',
                   help="keep the dataset on the GPU and gather every batch there (data_loading/resident.py); CUDA devices only")
    p.add_argument('--ensemble', action='store_true',
                   help="train all --repeat SynthesisLite models in one pass (models/synthesis_ensemble_trainer.py); implies "
                        "--resident; needs both classifier checkpoints, a CUDA device and a single process")
    p.add_argument('--f0_metrics', action='store_true',
                   help="compare the F0 contours of the original and the synthesised waveforms of --audio_dir (utils/audio.py "
                        "yin_f0_batch, utils/metrics.py compute_f0_metrics); writes f0_metrics.json and f0_tracks.npz there")
    return p


def _build_classifier(name: str, n_channels: int, seq_length: int, n_classes: int, kwargs: dict, role: str):
    if name == 'ShallowNN':
        return ShallowNNClassifier(input_dim=n_channels * seq_length, n_classes=n_classes, **kwargs)
    if name == 'logistic':
        return LogisticRegressionClassifier(input_dim=n_channels * seq_length, n_classes=n_classes, **kwargs)
    if name == 'CNN':
        return CNNClassifier(input_channels=n_channels, input_length=seq_length, n_classes=n_classes, **kwargs)
    if name == 'CNNRNN':
        return CNNRNNClassifier(input_channels=n_channels, input_length=seq_length, n_classes=n_classes, **kwargs)
    raise ValueError(f"Unknown {role} model name: {name}. Supported models: CNN, ShallowNN, logistic, CNNRNN.")


def _mels_from_dataset(dataset, params, mel_kwargs) -> np.ndarray:
    """Mel targets: a pre-computed 'mel' array of the sample file, else the audio of every sample through
    ``utils.audio.audio_to_mel`` (reference train_synthesizer.py:189-201) - on a CUDA device the whole ``audio`` array in one
    ``audio_to_mel_batch`` call, on 'cpu' trial by trial on the host."""
    if 'mel' in dataset:
        return np.asarray(dataset['mel'], dtype=np.float32)
    from .utils.audio import audio_to_mel, audio_to_mel_batch
    if 'cuda' in str(params.device):
        return audio_to_mel_batch(np.asarray(dataset['audio']), params.audio_sampling_rate, mel_kwargs=mel_kwargs,
                                  device=params.device)
    return np.array([audio_to_mel(audio, params.audio_sampling_rate, mel_kwargs=mel_kwargs) for audio in dataset['audio']])


ENSEMBLE_NEEDS = ("--ensemble needs --synthesis_model_name SynthesisLite, both classifier checkpoints (--tone_model_path and "
                  "--syllable_model_path), a CUDA device and a single process (no torchrun / process group)")


def check_ensemble(params: Namespace) -> bool:
    """Is the one-pass ensemble asked for?  Raises ``ValueError`` (stating the conditions) where it cannot run."""
    if not bool(getattr(params, 'ensemble', False)):
        return False
    unmet = []
    if params.synthesis_model_name != 'SynthesisLite':
        unmet.append(f"synthesis_model_name is '{params.synthesis_model_name}'")
    if getattr(params, 'tone_model_path', None) is None or getattr(params, 'syllable_model_path', None) is None:
        unmet.append("a classifier checkpoint is missing")
    if 'cuda' not in str(params.device):
        unmet.append(f"device is '{params.device}'")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 or parallel.world()[1] > 1:
        unmet.append("more than one process")
    if unmet:
        raise ValueError(f"{'; '.join(unmet)}: {ENSEMBLE_NEEDS}")
    return True


#: the F0 range of ``--f0_metrics``, Hz: below the lowest male and above the highest female speaking pitch
F0_FMIN, F0_FMAX = 60.0, 500.0


def check_f0_metrics(params: Namespace) -> bool:
    """Is ``--f0_metrics`` asked for?  Raises ``ValueError`` naming the flag where there is no ``--audio_dir`` to work in."""
    if not bool(getattr(params, 'f0_metrics', False)):
        return False
    if not getattr(params, 'audio_dir', None):
        raise ValueError("--f0_metrics needs --audio_dir: it tracks F0 on the waveforms written there")
    return True


def write_f0_metrics(waves: np.ndarray, n_audio: int, params: Namespace, mel_kwargs: dict) -> Optional[dict]:
    """F0 of the (2 n_audio, samples) waveforms - rows [0, n_audio) the originals, the rest the reconstructions, both out of
    the same mel inversion, so what differs is the model's - on the frames of the mel front end (``n_fft``, ``hop_length``),
    60 - 500 Hz; ``compute_f0_metrics`` of the two halves -> ``f0_metrics.json``, the tracks -> ``f0_tracks.npz`` (rows as
    ``waves``).  On a CUDA device one ``yin_f0_batch`` call, on 'cpu' ``yin_f0`` clip by clip."""
    from .utils.audio import F0Track, yin_f0, yin_f0_batch
    from .utils.metrics import compute_f0_metrics
    if n_audio < 1 or waves.shape[1] < 1:
        print("f0_metrics: no waveform to track (no audio sample, or mel spectrograms of a single frame)")
        return None
    sr = float(params.audio_sampling_rate)
    kw = dict(frame_length=int(mel_kwargs.get("n_fft", 2048)), hop_length=mel_kwargs.get("hop_length"))
    if 'cuda' in str(params.device):
        track = yin_f0_batch(waves, sr, F0_FMIN, F0_FMAX, device=params.device, **kw)
    else:
        track = F0Track(*(np.stack(col) for col in zip(*(yin_f0(w, sr, F0_FMIN, F0_FMAX, **kw) for w in waves))))
    metrics = compute_f0_metrics(F0Track(*(t[:n_audio] for t in track)), F0Track(*(t[n_audio:] for t in track)))
    np.savez(os.path.join(params.audio_dir, 'f0_tracks.npz'), **track._asdict())
    with open(os.path.join(params.audio_dir, 'f0_metrics.json'), 'w') as f:
        json.dump(metrics, f, indent=1)
    print(f"F0 of the synthesised against the original waveforms ({metrics['n_voiced']} frames voiced in both): "
          f"RMSE {metrics['f0_rmse_cents']:.1f} cents, correlation {metrics['f0_corr']:.3f}, "
          f"gross pitch error {metrics['gross_pitch_error']:.3f}, voicing error {metrics['voicing_error']:.3f}")
    return metrics


def train(params: Namespace) -> dict:
    """Body of the reference script (:137-400) on the MI355X trainer.  Returns the result row."""
    if not os.path.exists(params.sample_path):
        raise FileNotFoundError(f"Data file '{params.sample_path}' does not exist.")
    f0_metrics = check_f0_metrics(params)
    ensemble = check_ensemble(params)
    # data parallel: one process per GPU under torchrun (RANK / LOCAL_RANK / WORLD_SIZE).  The process group
    # is created before any GPU call; rank r trains on cuda:LOCAL_RANK, every rank sees the same loaders
    # (same seeds) and takes its row shard of each batch inside SynthesisTrainer; only rank 0 writes files.
    rank, world, local = parallel.init_from_env()
    if world > 1:
        params.device = f"cuda:{local}"
    if 'cuda' in params.device and not torch.cuda.is_available():
        raise RuntimeError("CUDA is not available. Please use 'cpu' as device.")
    chief = rank == 0
    say = print if chief else (lambda *a, **k: None)
    for d in (params.figure_dir, params.audio_dir, os.path.dirname(params.result_file)):
        if chief and d and not os.path.exists(d):
            os.makedirs(d)
    with open(params.channel_file, 'r') as f:
        channel_selections = json.load(f)
    non_disc = select_non_discriminative_channels(channel_selections,
                                                  ['tone_discriminative', 'syllable_discriminative'])
    say('Found {} non-discriminative channels.'.format(len(non_disc)))
    with open(params.config_file, 'r') as f:
        config = json.load(f)
    mel_kwargs = config['mel_kwargs']
    tone_dynamic_mapping = config['tone_dynamic_mapping']
    n_syllables, n_tones = config['n_syllables'], config['n_tones']

    dataset = np.load(params.sample_path)
    ecog = dataset['ecog']
    syl_channels, tone_channels = channel_selections['syllable_discriminative'], channel_selections['tone_discriminative']
    # resident: ecog is stored once on the device and read through the three channel lists by the batch gather; the three
    # host copies ecog[:, channels, :] are not made
    resident = (bool(getattr(params, 'resident', False)) or ensemble) and 'cuda' in str(params.device)
    if resident:
        n_samples, n_timepoints = ecog.shape[0], ecog.shape[2]
        n_channels, n_syl_channels, n_tone_channels = len(non_disc), len(syl_channels), len(tone_channels)
    else:
        ecog_non = ecog[:, non_disc, :]
        ecog_syl = ecog[:, syl_channels, :]
        ecog_tone = ecog[:, tone_channels, :]
        n_samples, n_channels, n_timepoints = ecog_non.shape
        n_syl_channels, n_tone_channels = ecog_syl.shape[1], ecog_tone.shape[1]
    mels = _mels_from_dataset(dataset, params, mel_kwargs)
    say('Number of Mel spectrogram coefficients', mels.shape[1:])
    mels_dim = mels.shape[1]
    seq_length = ecog.shape[2]

    syl_kwargs = config.get('syllable_model_kwargs', {})
    tone_kwargs = config.get('tone_model_kwargs', {})
    syllable_model = _build_classifier(params.syllable_model_name, n_syl_channels, seq_length, n_syllables,
                                       syl_kwargs, "syllable")
    tone_model = _build_classifier(params.tone_model_name, n_tone_channels, seq_length, n_tones, tone_kwargs, "tone")
    if params.syllable_model_path is not None:
        syllable_model.load_state_dict(torch.load(params.syllable_model_path))
    if params.tone_model_path is not None:
        tone_model.load_state_dict(torch.load(params.tone_model_path))
    train_classifiers = not (params.syllable_model_path is not None and params.tone_model_path is not None)

    if params.verbose > 0:
        say(f"Prepared {n_samples} ECoG samples with shape {ecog.shape[1:]}")
    if resident:
        from .data_loading.resident import ResidentDataset
        ecog_t = torch.tensor(ecog, dtype=torch.float32)
        tds = ResidentDataset([(ecog_t, non_disc), (ecog_t, syl_channels), (ecog_t, tone_channels),
                               (torch.tensor(mels, dtype=torch.float32), None)], device=params.device)
    else:
        tds = TensorDataset(torch.tensor(ecog_non, dtype=torch.float32), torch.tensor(ecog_syl, dtype=torch.float32),
                            torch.tensor(ecog_tone, dtype=torch.float32), torch.tensor(mels, dtype=torch.float32))

    mcds, losses = [], []
    np.random.seed(params.seed)
    seeds = np.random.randint(0, 10000, params.repeat)
    model = None
    if ensemble:
        # every seed in one pass.  The per-seed prologue consumes each seed's random stream in the order of the loop below
        # (set_seeds, split_dataset, model construction): batches, initial weights and dropout masks are the loop's
        from .models.synthesis_ensemble_trainer import SynthesisEnsembleTrainer
        all_loaders, models, entered = [], [], []
        for seed in seeds:
            set_seeds(int(seed))
            all_loaders.append(split_dataset(tds, [params.train_ratio, 1 - params.train_ratio], shuffling=[True, False],
                                             batch_size=params.batch_size, seed=int(seed), resident=True))
            models.append(SynthesisLite(output_dim=mels_dim, n_channels=n_channels, n_timepoints=n_timepoints))
            entered.append(torch.get_rng_state())            # where the seed's ``train`` is entered
        trainer = SynthesisEnsembleTrainer(models, tone_model, syllable_model, tone_dynamic_mapping,
                                           seeds=[int(s) for s in seeds], device=params.device, learning_rate=params.lr,
                                           verbose=chief and params.verbose > 0, train_classifiers=train_classifiers,
                                           rng_states=entered)
        if params.verbose > 0:
            say(f"Training {len(models)} synthesizers in one pass with seeds {seeds.tolist()}...")
        histories = trainer.train_loaders([lo[0] for lo in all_loaders], params.epochs, verbose=chief and params.verbose > 1)
        evaluated = trainer.evaluate([lo[1] for lo in all_loaders])
        for i, (history, (mcd, recon_mels, origin_mels)) in enumerate(zip(histories, evaluated)):
            mcds.append(mcd)
            if params.verbose > 0:
                say(f"Finished trial {i+1} / {params.repeat}. MCD: {mcd:.4f} dB")
            losses.append([loss for loss, _ in history])
        model = models[-1]
    for i, seed in enumerate(() if ensemble else seeds):
        set_seeds(int(seed))
        ratios = [params.train_ratio, 1 - params.train_ratio]
        loaders = split_dataset(tds, ratios, shuffling=[True, False], batch_size=params.batch_size, seed=int(seed),
                                resident=resident)
        if params.synthesis_model_name == 'SynthesisLite':
            model = SynthesisLite(output_dim=mels_dim, n_channels=n_channels, n_timepoints=n_timepoints)
        elif params.synthesis_model_name == 'SynthesisFull':
            model = SynthesisModelCNN(output_dim=mels_dim, n_channels=n_channels, n_timepoints=n_timepoints)
        else:
            raise ValueError(f"Unknown synthesizer model name: {params.synthesis_model_name}. "
                             f"Supported models: {synthesis_models}.")
        trainer = SynthesisTrainer(synthesize_model=model, syllable_model=syllable_model, tone_model=tone_model,
                                   device=params.device, tone_dynamic_mapping=tone_dynamic_mapping,
                                   learning_rate=params.lr, verbose=chief and params.verbose > 0 and i == 0,
                                   train_classifiers=train_classifiers)
        if params.verbose > 0:
            say(f"Training synthesizer with seed {seed}...")
        history = trainer.train(loaders[0], params.epochs, verbose=chief and params.verbose > 1)
        mcd, recon_mels, origin_mels = trainer.evaluate(loaders[1])
        mcds.append(mcd)
        if params.verbose > 0:
            say(f"Finished trial {i+1} / {params.repeat}. MCD: {mcd:.4f} dB")
        losses.append([loss for loss, _ in history])

    mean_mcd, std_mcd = float(np.mean(mcds)), float(np.std(mcds))
    total_size = model.get_nparams() + syllable_model.get_nparams() + tone_model.get_nparams()
    results = {
        'model_name': params.model_name, 'model_size': total_size,
        'tone_model': params.tone_model_name, 'tone_model_kwargs': str(tone_kwargs),
        'syllable_model': params.syllable_model_name, 'syllable_model_kwargs': str(syl_kwargs),
        'subject': params.subject_id, 'mel_kwargs': str(mel_kwargs), 'seeds': str(seeds.tolist()),
        'batch_size': params.batch_size, 'epochs': params.epochs, 'learning_rate': params.lr,
        'mcd_mean': mean_mcd, 'mcd_std': std_mcd, 'all_mcds': str(mcds),
    }
    results['losses'] = losses
    if not chief:
        return results
    df = pd.DataFrame([{k: v for k, v in results.items() if k != 'losses'}])
    if os.path.exists(params.result_file):
        df.to_csv(params.result_file, mode='a', header=False, index=False)
    else:
        df.to_csv(params.result_file, mode='w', header=True, index=False)
    print('Saved results to ', params.result_file)
    print(f"-------- Training completed over {params.repeat} runs --------")
    print(f"MCD (Mel-Cepstral Distortion): {mean_mcd:.4f} dB ± {std_mcd:.4f} dB")
    if params.figure_dir:
        path = os.path.join(params.figure_dir, 'training_losses.png')
        plot_training_losses(losses, figure_path=path)
        print("Saved training losses figure to ", path)
    if params.audio_dir:
        np.savez(os.path.join(params.audio_dir, 'mels.npz'), origin=origin_mels[:10], recon=recon_mels[:10])
        # the first samples as audio (reference :408-428): Griffin-Lim inversion of the original / synthesised dB mels - on a
        # CUDA device all of them in one mel_to_audio_batch call, on 'cpu' trial by trial on the host
        from scipy.io.wavfile import write as write_wave
        from .utils.audio import mel_to_audio, mel_to_audio_batch
        stft_kw = {k: mel_kwargs[k] for k in ("n_fft", "hop_length", "win_length", "fmin", "fmax") if k in mel_kwargs}
        n_audio = min(int(getattr(params, "n_audio_samples", 10)), len(origin_mels))
        waves = None
        if 'cuda' in str(params.device) and n_audio > 0:
            # one call for all selected originals and reconstructions: rows [0, n_audio) origin, [n_audio, 2 n_audio) recon
            both = np.concatenate([np.asarray(origin_mels[:n_audio]).reshape(n_audio, -1),
                                   np.asarray(recon_mels[:n_audio]).reshape(n_audio, -1)])
            waves = mel_to_audio_batch(both, mel_kwargs['n_mels'], audio_sampling_rate=params.audio_sampling_rate,
                                       device=params.device, **stft_kw)
        host_waves = [[], []]
        for i in range(n_audio):
            for k, (tag, mel) in enumerate((("origin", origin_mels[i]), ("recon", recon_mels[i]))):
                wave = waves[k * n_audio + i] if waves is not None else \
                    mel_to_audio(np.asarray(mel), mel_kwargs['n_mels'], audio_sampling_rate=params.audio_sampling_rate, **stft_kw)
                host_waves[k].append(wave)
                if wave.size == 0:          # a single mel frame inverts to zero samples (centred STFT)
                    continue
                path = os.path.join(params.audio_dir, f'{tag}_audio_{i}.wav')
                write_wave(path, int(params.audio_sampling_rate), wave)
                print(f"Saved {tag} audio to ", path)
        if f0_metrics:
            if waves is None:
                waves = np.array(host_waves[0] + host_waves[1]).reshape(2 * n_audio, -1) if n_audio else np.zeros((0, 0))
            write_f0_metrics(np.asarray(waves), n_audio, params, mel_kwargs)
    return results


def run(config: dict) -> Optional[str]:
    """YAML entry for ``main.py``: ``config['training']['params']`` holds the CLI flag names
    (nested ``io`` / ``training`` / ``experiment`` groups are flattened)."""
    stage = config.get("training", config)
    raw = dict(stage.get("params", stage))
    flat = {}
    for k, v in raw.items():
        if isinstance(v, dict) and k in ("io", "training", "experiment", "model"):
            flat.update(v)
        else:
            flat[k] = v
    defaults = vars(build_parser().parse_args(
        ['--sample_path', '_', '--subject_id', '_', '--result_file', '_', '--model_name', '_',
         '--synthesis_model_name', '_', '--syllable_model_name', '_', '--tone_model_name', '_']))
    required = ['sample_path', 'subject_id', 'result_file', 'model_name', 'synthesis_model_name',
                'syllable_model_name', 'tone_model_name']
    missing = [k for k in required if k not in flat]
    if missing:
        raise KeyError(f"train_synthesizer.run: missing training params {missing}")
    defaults.update({k: v for k, v in flat.items() if k in defaults})
    train(Namespace(**defaults))
    return os.path.dirname(defaults['result_file']) or None


if __name__ == '__main__':
    train(build_parser().parse_args())
