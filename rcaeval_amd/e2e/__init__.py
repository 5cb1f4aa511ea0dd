"""RCA method plug-ins on the MI355X engine (mirror of ``RCAEval/e2e``).

``rca`` mirrors the reference wrapper (``RCAEval/e2e/__init__.py:21-31``): an exception
raised by the method returns the dummy ranking ``preprocess(data, dataset).columns``. That
covers what the reference's methods raise on their data — ``ValueError`` from a singular
sub-matrix or a math domain error (which the engine raises as ``ValueError`` too), pandas /
numpy errors — and the one data-driven engine outcome, a list overflow that survived the
engine's own reruns (``PcgError`` PCG_ERR_OVERFLOW, with a warning). Engine FAULTS propagate:
``EngineUnavailable`` (no GPU, library missing) and ``PcgError`` with PCG_ERR_INVALID / OOM /
HIP / RCCL / PEER. A sticky device fault or an OOM would otherwise score that case and every
later case of an RQ2 run as dummy rankings, silently corrupting the benchmark.
"""
from __future__ import annotations

import functools
import warnings

from .._lib import PCG_ERR_OVERFLOW, EngineUnavailable, PcgError
from ..io.time_series import preprocess


def rca(func):
    """Tolerate method failures like the reference's ``@rca`` (``e2e/__init__.py:21-31``)."""
    @functools.wraps(func)
    def wrapper(*args, **kwargs):
        try:
            return func(*args, **kwargs)
        except EngineUnavailable:
            raise
        except PcgError as e:
            if e.code != PCG_ERR_OVERFLOW:
                raise                       # an engine fault, not an outcome of this case's data
            warnings.warn(f"{func.__name__}: engine error, dummy ranks returned: {e}")
            return _dummy(args, kwargs)
        except Exception:
            return _dummy(args, kwargs)
    return wrapper


def _dummy(args, kwargs):
    """The reference's fallback ranking: the preprocessed column names."""
    data = preprocess(data=args[0], dataset=kwargs.get("dataset"), dk_select_useful=False)
    names = data.columns.to_list()
    return {"adj": [], "node_names": names, "ranks": names}


from .baro import baro, baro_batch, nsigma, nsigma_batch, robust_scaler  # noqa: E402
from .circa import circa  # noqa: E402
from .cloudranger import cloudranger  # noqa: E402
from .pc_pagerank import cmlp_pagerank, pc_pagerank, pc_pagerank_batch  # noqa: E402
from .fci_pagerank import fci_pagerank  # noqa: E402
from .ges_pagerank import fges_pagerank, fges_randomwalk  # noqa: E402
from .granger_pagerank import granger_pagerank  # noqa: E402
from .lingam_pagerank import micro_diag  # noqa: E402
from .microcause import microcause  # noqa: E402
from .pc_randomwalk import fci_randomwalk, granger_randomwalk, pc_randomwalk  # noqa: E402

__all__ = ["rca", "baro", "baro_batch", "circa", "cloudranger", "cmlp_pagerank", "fci_pagerank", "fci_randomwalk", "fges_pagerank",
           "fges_randomwalk", "granger_pagerank", "granger_randomwalk", "micro_diag", "microcause", "nsigma",
           "nsigma_batch", "pc_pagerank", "pc_pagerank_batch", "pc_randomwalk", "robust_scaler"]
