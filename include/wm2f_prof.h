/*
 * wm2f_prof.h -- additions of the PROFILING build of the library (libwm2f_prof.so = the same sources compiled with
 * -DWM2F_PROFILING; `python -m weed_instance_segmentation_amd._build --prof`).  Used by tools/ only: never by the
 * product path, the tests' parity checks or bench.py.  It exports everything include/wm2f.h declares, plus:
 *
 *   - wm2f_msdeform_fwd_v accepts, beside the production variants 0 / 1 / 2 / 4:
 *       62                      LDS-window kernel in slab-major work order (valid outputs)
 *     timing ablations, whose OUTPUTS ARE NOT VALID
 *       12 / 22 / 32 / 42 / 52  LDS-window kernel: staging only, gather only, no operand loads, no LDS reads, neither
 *       44                      streaming quad kernel without LDS reads
 *     a stamped build (valid outputs)
 *       74                      streaming quad kernel with in-kernel time stamps
 *     Every other number returns WM2F_EUNSUPPORTED, as in the production library.
 *   - wm2f_msdeform_fused_lanes_fwd reads WM2F_K1_STAMP (1: the stamped kernel) and WM2F_K1_MODE on every launch: 800 slab
 *     order, 807 slab order stamped, and the slab-order kernel's timing ablations (OUTPUTS NOT VALID) 814 no LDS reads,
 *     815 no window DMA, 816 no operand loads / stores, 820 operand loads from one hot record; any other value is refused
 *     (tools/k1_slab_inmodel.py, tools/k1_stamps.py)
 *   - wm2f_msdeform_rows_bwd reads WM2F_K1_LW_THREADS: 512 / 768 = 8 / 12 waves per workgroup in the row-gradient kernel,
 *     1 / 2 = that kernel without window staging / staging only (OUTPUTS NOT VALID), 3 = that kernel alone (grad_value not
 *     computed)   (tools/probes/k1_rows_bench.py)
 *   - K2 / K3 read their experiment knobs from the environment on every launch
 *       WM2F_K2_QTILES, WM2F_K2_WG_TARGET, WM2F_K2_FULL, WM2F_K2_QSPLIT, WM2F_K3_DBG   (tools/kbench.py)
 *   - wm2f_token_linear_split_fwd reads on every launch   (tools/kbench.py --prof --only tgs)
 *       WM2F_TGS_ABL  timing ablations of the shipped kernel, whose OUTPUTS ARE NOT VALID: 1 no epilogue stores, 2 no
 *                     epilogue loads (residual and pos read as zero), 4 no MFMAs; any other value is refused
 *       WM2F_TGS_OPT  0: the LayerNorm epilogue with its residual / pos loads one batch at a time, as before section 13.2
 *                     (valid outputs, the same bits as the shipped kernel); 1 or unset: the shipped kernel
 *   - wm2f_token_ffn_split_fwd reads on every launch   (tools/kbench.py --prof --only ffn)
 *       WM2F_FFN_ABL  timing ablations whose OUTPUTS ARE NOT VALID: 1 no epilogue stores, 4 no MFMAs; any other value is refused
 *   - wm2f_conv3x3_split_fwd / _fwd_p read on every launch   (tools/conv3x3_configs.py --ablation)
 *       WM2F_C3_ABL   timing ablations whose OUTPUTS ARE NOT VALID (three pieces, no statistics): 1 splits x at tap 0 of
 *                     each channel block only and feeds those pieces to taps 1 .. 8, 2 also drops the x loads of taps
 *                     1 .. 8; any other value is refused
 *   - the stamp buffer below: a __device__ global, i.e. the global mutable state the production library forbids.
 */
#ifndef WM2F_PROF_H
#define WM2F_PROF_H

#include "wm2f.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Variant 74 of wm2f_msdeform_fwd_v stamps s_memtime in the second tile of every workgroup: EVERY wave into
 * [wave][slot] -- gather waves slots 0-9, loader waves slots 10-15.  This copies the stamps to HOST memory (int64 [8192 workgroups][160] = [8192][10 waves][16],
 * n_bytes <= 10 MiB).  Synchronous; no reference counterpart. */
int wm2f_debug_stamps(void* host_dst, int64_t n_bytes);

#ifdef __cplusplus
}
#endif
#endif /* WM2F_PROF_H */
