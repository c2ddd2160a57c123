"""The block driver of the preprocess stage (counterpart of reference preprocess/pipelines/subject_block.py).

Input tree::

    root_dir/<subject_dir>/HS<subject>-<block>/        one directory per block (``B<block>`` is read too)

``run`` walks subjects and blocks, loads a block with the io module, runs the configured steps of every modality through
the preprocessor, and writes ``<output_dir>/<setup>/subject_<id>/B<block>_<modality>.npz`` plus ``<setup>/config.yaml``.

Kept from the reference: how a block number is read off a directory name (and the message for one that does not parse),
``subject_ids`` defaulting to 1..n, the setup name (``generate_setup_name``), ``figures/subject_<id>/block_<id>/``, the
progress lines, the returned setup directory.  The block parameters are the io parameters without ``root_dir`` /
``output_dir`` plus ``block_id`` and ``subject_id`` (the reference lists the two directories as ``exclude_keys``, which in
its ``dict_to_namespace`` leaves them in; they are left out here, as that list says).

Changed on purpose:
  * block directories are visited in ``sorted(os.listdir(...))`` order, so the order of the work and of the progress lines
    does not depend on the file system (sample collection makes the same choice);
  * ``config.yaml`` is dumped from plain dicts, so it stays ``yaml.safe_load``-able when a parameter is nested (the
    reference dumps ``vars(Namespace)``, which writes a nested Namespace as a Python object tag).

On the device the stage adds no arithmetic - that is the signal kernels' - but residency.  Optional pipeline parameters:
  ``resident`` (default true)        every modality that has steps is uploaded once, flows through the preprocessor as a CUDA
                                     tensor and comes back once, for ``save_block``.  A modality without steps is never
                                     uploaded and is written back as it was loaded.  Used only with a preprocessor whose
                                     ``preprocess_modalities`` takes ``resident``; any other gets the host arrays.
  ``shard_channels`` (default false) passed to such a preprocessor.
  ``figures`` (default true)         false: the preprocessor gets ``figure_dir=None`` and draws nothing.
  ``keep_resident`` (default false)  the saved blocks are also kept for the sample-collection stage of the same process
                                     (``preprocess/handover.py``); the files are written all the same.
  ``diagnostics`` (default false)    the input of the first step and the output of every step of a modality are summarised on
                                     the device (``utils/diagnostics.py``: Welch PSD, mean and std per second) and written to
                                     ``<setup>/diagnostics/subject_<id>/block_<id>/<modality>/step<i>_<module>.npz``
                                     (``step0_input`` is the input).  Needs a preprocessor whose ``preprocess_modalities`` takes
                                     ``diagnostics_dir``; refused with ``shard_channels``, as per-step figures are.  Absent or
                                     false: nothing is computed and no directory is made."""
from __future__ import annotations

import hashlib
import inspect
import os
from typing import Any, Dict

import numpy as np
import yaml

from .. import handover
from ...utils.config import dict_to_namespace, namespace_to_dict

release = handover.release


def get_block_id(dirname: str):
    """The block number of a directory name: what follows the last ``-``, an optional ``B`` removed.  None (and a message)
    for a name that does not end in a number."""
    try:
        return int(dirname.split('-')[-1].replace('B', ''))
    except ValueError:
        print(
            f"Skipping directory '{dirname}' as it does not match expected format.",
            "Expected format: 'HS<subject_id>-<block_id>'.",
        )
        return None


def iter_blocks(root_dir: str, subject_dirs, subject_ids=None):
    """Yield ``(subject_id, block_id, block_path)``, a subject's entries in sorted order."""
    if subject_ids is None:
        subject_ids = [i + 1 for i in range(len(subject_dirs))]
    for subject_id, subject_dir in zip(subject_ids, subject_dirs):
        subject_path = os.path.join(root_dir, subject_dir)
        for dir_name in sorted(os.listdir(subject_path)):
            block_id = get_block_id(dir_name)
            if block_id is None:
                continue
            yield subject_id, block_id, os.path.join(subject_path, dir_name)


def generate_setup_name(modalities_cfg: Dict[str, Any]) -> str:
    """``<last component of every step module, joined by "__">_<md5 of "<module>_<params>" joined by "_", 6 digits>`` over
    the steps of all modalities in config order; ``raw`` without steps.  Bit for bit the reference's name: the digest is
    taken over ``str(dict)`` of the step parameters."""
    steps = []
    for mod_cfg in modalities_cfg.values():
        steps.extend(mod_cfg.get("preprocessing", {}).get("steps", []))
    if not steps:
        return "raw"
    readable = "__".join(step["module"].split(".")[-1] for step in steps)
    setup_str = "_".join(f"{step['module']}_{step.get('params', {})}" for step in steps)
    return f"{readable}_{hashlib.md5(setup_str.encode()).hexdigest()[:6]}"


def _takes(function, name: str) -> bool:
    try:
        params = inspect.signature(function).parameters
    except (TypeError, ValueError):
        return False
    return name in params or any(p.kind is inspect.Parameter.VAR_KEYWORD for p in params.values())


def _upload(data_dict: dict, modalities_cfg: Dict[str, Any]) -> None:
    """Every modality that has steps -> CUDA tensor, in place; one copy each."""
    import torch
    for modality, cfg in modalities_cfg.items():
        if not cfg.get("preprocessing", {}).get("steps") or modality not in data_dict:
            continue
        value = data_dict[modality]
        if not isinstance(value, torch.Tensor):
            value = torch.from_numpy(np.ascontiguousarray(value))
        data_dict[modality] = value.to("cuda")


def run(pipeline_params, io_params, io_module, preprocessor_module, modalities_cfg) -> str:
    setup_dir = os.path.join(io_params.output_dir, generate_setup_name(modalities_cfg))
    os.makedirs(setup_dir, exist_ok=True)
    figure_root = os.path.join(setup_dir, "figures")
    os.makedirs(figure_root, exist_ok=True)
    with open(os.path.join(setup_dir, "config.yaml"), "w") as f:
        yaml.dump({"preprocess": {"pipeline": namespace_to_dict(pipeline_params), "io": namespace_to_dict(io_params),
                                  "modalities": namespace_to_dict(modalities_cfg)}}, f)

    figures = bool(getattr(pipeline_params, "figures", True))
    keep_resident = bool(getattr(pipeline_params, "keep_resident", False))
    extra = {}
    if _takes(preprocessor_module.preprocess_modalities, "resident"):
        extra["resident"] = bool(getattr(pipeline_params, "resident", True))
    if _takes(preprocessor_module.preprocess_modalities, "shard_channels"):
        extra["shard_channels"] = bool(getattr(pipeline_params, "shard_channels", False))
    diagnostics = bool(getattr(pipeline_params, "diagnostics", False))
    if diagnostics and bool(getattr(pipeline_params, "shard_channels", False)):
        raise ValueError("subject_block: 'diagnostics' needs the whole recording; not available with shard_channels")
    if diagnostics and not _takes(preprocessor_module.preprocess_modalities, "diagnostics_dir"):
        raise ValueError("subject_block: 'diagnostics' needs a preprocessor whose preprocess_modalities takes diagnostics_dir")

    for subject_id, block_id, block_path in iter_blocks(io_params.root_dir, pipeline_params.subject_dirs,
                                                        getattr(pipeline_params, "subject_ids", None)):
        print(f"Processing block {block_id} of subject {subject_id}...")
        data_dict = io_module.load_block(block_path)
        block_params = dict_to_namespace({**{k: v for k, v in vars(io_params).items() if k not in ("root_dir", "output_dir")},
                                          "block_id": block_id, "subject_id": subject_id})
        block_figure_dir = os.path.join(figure_root, f"subject_{subject_id}", f"block_{block_id}")
        os.makedirs(block_figure_dir, exist_ok=True)
        if extra.get("resident"):
            _upload(data_dict, modalities_cfg)
        if diagnostics:
            extra["diagnostics_dir"] = os.path.join(setup_dir, "diagnostics", f"subject_{subject_id}", f"block_{block_id}")
        preprocessor_module.preprocess_modalities(data_dict, modalities_cfg, block_params,
                                                  figure_dir=block_figure_dir if figures else None, **extra)
        io_module.save_block(setup_dir, subject_id, block_id, data_dict)
        if keep_resident:
            handover.register(os.path.join(setup_dir, f"subject_{subject_id}"), block_id, data_dict)
    return setup_dir
