"""Analysis of trained policies: checkpoint roll-outs that record the network's activations, their rendering, PCA of a recorded feature and the
PCA-progression video (track_mjx/analysis of the reference; text in plots and mp4 output are not built)."""
