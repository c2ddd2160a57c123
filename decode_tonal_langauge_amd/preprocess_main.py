"""The preprocess stage (counterpart of reference preprocess_main.py): the first stage of the YAML pipeline.

``run(config)`` / ``main(config_path)`` read ``preprocess.params``:

  pipeline      ``{module, params}``: what walks the raw tree; ``preprocess.pipelines.subject_block`` takes ``subject_dirs``,
                optional ``subject_ids`` and this build's optional ``resident`` / ``shard_channels`` / ``figures`` /
                ``keep_resident``
  io            ``{module, params}``: ``load_block`` / ``save_block``; params ``root_dir``, ``output_dir`` (anything else
                reaches every step through the block parameters)
  preprocessor  ``{module}``, default ``preprocess.preprocessor``
  modalities    ``<name>: {type: signal, preprocessing: {steps: [{module, params}, ...]}}``

and call ``pipeline_module.run(pipeline_params, io_params, io_module, preprocessor_module, modalities_cfg)``.  Both return
the pipeline's output directory: the ``str`` that makes ``main.run_pipeline`` offer it to ``sample_collection`` as
``recording_dir``.  The reference has ``main(path)`` only and returns nothing, so ``main.py``'s default ``function: run``
fails on it; ``run`` is this build's addition.

Module names of the reference layout resolve to this package (``preprocess.preprocessor.resolve_module``); any other dotted
name is imported as it is."""
from __future__ import annotations

import sys

from .preprocess.preprocessor import resolve_module
from .utils.config import dict_to_namespace, load_config


def run(config: dict) -> str:
    pre_cfg = (config.get("preprocess") or {}).get("params", {})
    pipeline_cfg = pre_cfg.get("pipeline", {})
    io_cfg = pre_cfg.get("io", {})
    preprocessor_cfg = pre_cfg.get("preprocessor", {"module": "preprocess.preprocessor"})
    modalities_cfg = pre_cfg.get("modalities", {})
    for what, cfg in (("pipeline", pipeline_cfg), ("io", io_cfg), ("preprocessor", preprocessor_cfg)):
        if not cfg.get("module"):
            raise KeyError(f"preprocess.params.{what}.module is missing from the configuration")

    pipeline_module = resolve_module(pipeline_cfg["module"])
    preprocessor_module = resolve_module(preprocessor_cfg["module"])
    io_module = resolve_module(io_cfg["module"])

    pipeline_params = dict_to_namespace(pipeline_cfg.get("params", {}))
    io_params = dict_to_namespace(io_cfg.get("params", {}))
    return pipeline_module.run(pipeline_params, io_params, io_module, preprocessor_module, modalities_cfg)


def main(config_path: str) -> str:
    return run(load_config(config_path))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit("Usage: python -m decode_tonal_langauge_amd.preprocess_main <config.yaml>")
    main(sys.argv[1])
