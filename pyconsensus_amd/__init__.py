"""pyconsensus_amd -- MI355X-native Oracle.consensus() (PCA path) behind the pyconsensus API.

    from pyconsensus_amd import Oracle
    Oracle(reports, event_bounds=..., reputation=...).consensus()

Batched Monte Carlo rounds: :func:`consensus_batched`; rounds of different shapes in one launch:
:func:`consensus_ragged`, and many Oracle problems at once: :func:`consensus_many`.  Single huge matrices,
row-sharded over GPUs: :func:`pyconsensus_amd.pipeline.consensus_matrix`.
Monte Carlo trajectories generated, run and scored on the device: :func:`simulate`
(with :func:`generate`, :func:`generate_host` and the metric names :data:`METRICS`; the
module's other names: ``from pyconsensus_amd.simulate import ...``); a whole study, cells of
different shapes, rates and seeds, in one call: :func:`sweep` over a cell list or a :func:`grid`;
with error bars, liar-detection metrics and paired differences between cells: :func:`study`.
"""
__version__ = "0.1.0"

from .batched import consensus_batched, consensus_ragged  # noqa: E402,F401
from .oracle import Oracle  # noqa: E402,F401
from .many import consensus_many  # noqa: E402,F401
from .simulate import METRICS, generate, generate_host, grid, simulate, study, sweep  # noqa: E402,F401
