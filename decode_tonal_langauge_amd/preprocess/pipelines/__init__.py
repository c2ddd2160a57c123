"""Pipelines of the preprocess stage: what walks the raw tree and drives the preprocessor."""
