from pychain_amd.loss import ChainFunction, ChainLoss, ChainLossFunction, output_regularizer, weight_rows  # noqa: F401
from pychain_amd.loss import PosteriorTargets, occupancies, posterior_numerator, posterior_targets, posterior_xent, boost_rows  # noqa: F401
