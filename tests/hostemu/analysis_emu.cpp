// tests/hostemu/analysis_emu.cpp — TEST-ONLY: the host emulation of every analysis entry point of include/tmjx.h (tmjx_pca_*, tmjx_plot_strips,
// tmjx_readout_*, tmjx_kmeans_*, tmjx_hmm_*, tmjx_wavelet_bank*, tmjx_spectrogram*) as ONE translation unit and one library, under the header's own
// names: the emulation files include the header, so the compiler holds every signature to it.  Nothing in track_mjx_amd/ loads it.
#include "readout_emu.cpp"
#include "spectrogram_emu.cpp"
