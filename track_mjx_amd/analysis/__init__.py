"""Analysis of trained policies: checkpoint roll-outs that record the network's activations (track_mjx/analysis of the reference;
rendering, PCA and plotting are not built)."""
