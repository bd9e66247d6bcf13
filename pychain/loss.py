from pychain_amd.loss import ChainFunction, ChainLoss, ChainLossFunction, output_regularizer, weight_rows  # noqa: F401
