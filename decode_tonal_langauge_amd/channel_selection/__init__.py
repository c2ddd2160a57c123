"""Channel selection on the GPU (mirror of the reference's ``channel_selection`` package).

``active`` and ``discriminative`` are the two selector plugins (``run(data, params)`` /
``generate_figures(data, results, params, figure_dir)``), ``permutation`` a third that replaces their hand-set run length by
a label-permutation test of it; ``utils`` holds the host helpers of the reference plus ``anova_oneway``, the documented
low-level entry to the ANOVA kernels, ``kruskal_oneway`` / ``rank_columns``, its rank form (Kruskal-Wallis; the selectors'
key ``test: kruskal``), and the helpers of the permutation test."""
from .utils import anova_oneway, find_significant_channels, get_max_length, max_run_below  # noqa: F401
from .utils import permutation_p_values, permutation_runs, permutation_table  # noqa: F401
from .utils import kruskal_oneway, rank_columns  # noqa: F401
