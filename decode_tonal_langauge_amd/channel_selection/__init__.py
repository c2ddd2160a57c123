"""Channel selection on the GPU (mirror of the reference's ``channel_selection`` package).

``active`` and ``discriminative`` are the two selector plugins (``run(data, params)`` /
``generate_figures(data, results, params, figure_dir)``); ``utils`` holds the host helpers of the
reference plus ``anova_oneway``, the documented low-level entry to the ANOVA kernels."""
from .utils import anova_oneway, find_significant_channels, get_max_length, max_run_below  # noqa: F401
