"""Block readers and writers of the preprocess stage: ``load_block(block_path) -> dict``, ``save_block(...)``."""
