// vp_pv_transient.inc -- the transient-preserving locked time stretch's two kernels, each a file of its own (included by vp_stft.hip behind
// the locked time stretch, whose plan the second uses; both use the handle's tables, the transforms and stft_load_frame):
//   vp_stft_onset.inc          vp_k_stft_onset_flux: rectified spectral flux and spectral mass over the input's own frame grid
//   vp_stft_stretch_reset.inc  vp_k_stft_pv_stretch_lock_reset: vp_k_stft_pv_stretch_lock with a phase reset on flagged frames
// The host half -- picking the onsets, planning the positions around them -- is vp_onset_host.inc, included by vp_capi.hip.
#include "vp_stft_onset.inc"
#include "vp_stft_stretch_reset.inc"
