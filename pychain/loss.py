from pychain_amd.loss import ChainFunction, ChainLoss, ChainLossFunction, output_regularizer  # noqa: F401
