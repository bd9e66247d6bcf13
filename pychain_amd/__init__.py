"""pychain_amd: MI355X-native LF-MMI loss behind the pychain API.

    from pychain_amd import ChainGraph, ChainGraphBatch, ChainFunction, ChainLoss, viterbi_align, alignment_windows, output_regularizer

(`import pychain` resolves to the same objects through the alias package at the
repository root, so code written against the reference imports unchanged.)
"""
import os as _os


def _more_hardware_queues():
    """The loss runs on three streams and RCCL's collectives on a fourth; the HIP runtime maps streams onto four hardware queues by
    default, and a loss stream that shares a queue with RCCL's serialises behind it (measured: +37 % per step, bench.py).
    GPU_MAX_HW_QUEUES is read when the runtime initialises: set here - unless the user set it - while nothing has touched the
    device yet; a process that imports this package AFTER its first device call sets the variable itself."""
    if "GPU_MAX_HW_QUEUES" in _os.environ:
        return
    try:
        import torch
        if torch.cuda.is_initialized():
            return
    except Exception:
        pass
    _os.environ["GPU_MAX_HW_QUEUES"] = "16"


_more_hardware_queues()

from .graph import ChainGraph, ChainGraphBatch  # noqa: F401
from .loss import ChainFunction, ChainLoss, ChainLossFunction, numerator_xent, output_regularizer, weight_rows  # noqa: F401
from .loss import PosteriorTargets, occupancies, posterior_numerator, posterior_targets, posterior_xent, boost_rows  # noqa: F401
from .align import Alignment, alignment_windows, viterbi_align  # noqa: F401
from .smbr import SMBRFunction, SMBRLoss, expected_accuracy  # noqa: F401
from .arcs import ArcCounts, DenLogPartitionFunction, den_log_partition, expected_arc_counts  # noqa: F401
from .arcs import NumArcCounts, NumLogPartitionFunction, num_log_partition, expected_num_arc_counts  # noqa: F401
