// switches.h -- every RSRGAN_* environment variable the library looks at: one table, one reader.
//
// Columns: NAME (the variable is RSRGAN_<NAME>), field, kind, default, clamp, scope, meaning.
//   kind   BOOL  unset = default; set = (atoi(value) != 0).  Default 1 is "on unless 0", default 0 "off unless non-zero".
//          INT   unset = default; set = atoi(value), then the clamp.
//   clamp  ANY   none
//          MIN0  max(0, v)
//          W8    a worker count: 64..256 rounded down to a multiple of 8; anything else is the default
//   scope  handle   read when rsrgan_create constructs the Model (Model::sw): two handles of one process may differ
//          process  read once per process, all together, at the first use of any of them (switches())
//          call     read each time the call site runs (switch_now_<field>())
// RSRGAN_DPIPE used to be read at both scopes (handle: on / off at init; process: the level in d_backward); it is one handle-scope
// level now -- a handle created with it off never reached the second reading.  RSRGAN_GRAPH_DEBUG used to be "set at all"; it is an
// ordinary BOOL now (=0 is off).  The table is mirrored by hand in DESIGN.md "Runtime switches"; tests/test_switch_table.py
// holds the two together and checks that every name the tests and the benchmark flip is a row here.
#pragma once
#include <cstdlib>

namespace rsr {

// clang-format off
#define RSRGAN_SWITCHES(X) \
  X(GPERSIST,       gpersist,       INT,  3,    ANY,  handle,  "persistent generator recurrences (gpersist.hip): bit 0 the forward launch, bit 1 the BPTT; 0 = the launch-per-phase wavefront") \
  X(DPERSIST,       dpersist,       INT,  3,    ANY,  handle,  "persistent discriminator recurrences (dpersist.hip): bit 0 the forward launch, bit 1 the backward launch") \
  X(DFOLD,          dfold,          BOOL, 1,    ANY,  handle,  "folded small-cell recurrence of the discriminator (one launch per step); 0 = gates + projection") \
  X(TRAIL,          trail,          INT,  1,    ANY,  handle,  "the discriminator's BPTT trailing the generator's inside one launch (k_glstm_bwd_dt); 0 = two launches") \
  X(GRAPHS,         graphs,         BOOL, 1,    ANY,  handle,  "0 = RSRGAN_FLAG_GRAPH is ignored: every segment runs eagerly") \
  X(RCED_IMPLICIT,  rced_implicit,  BOOL, 1,    ANY,  handle,  "implicit-GEMM convolution for every R-CED layer it covers; 0 = patch-matrix GEMMs everywhere") \
  X(DPIPE,          dpipe,          INT,  0,    ANY,  handle,  "D(real) of the D-run ahead on the side stream: > 0 covers labels and lengths, >= 2 a noise_real tensor too (include/rsrgan.h)") \
  X(PAD_ROWS,       pad_rows,       BOOL, 1,    ANY,  process, "pad the batch to a multiple of 32 rows so that the persistent generator recurrences apply; 0 = the caller's row count") \
  X(DW_INKERNEL,    dw_inkernel,    BOOL, 1,    ANY,  process, "the discriminator's weight gradients inside its stand-alone BPTT launch; 0 = GEMM / column-sum launches behind it") \
  X(GP_NP_BWD,      gp_np_bwd,      BOOL, 1,    ANY,  process, "persistent BPTT of an unprojected generator (8 cells per workgroup); 0 = its BPTT takes the launch path") \
  X(GP_NP_NT,       gp_np_nt,       INT,  0,    ANY,  process, "gate tiles per workgroup of the unprojected generator's launches: 2 or 4; 0 = what the resident probe admits") \
  X(GP_NOPROJ,      gp_noproj,      BOOL, 1,    ANY,  process, "persistent forward recurrence for num_proj=None generators (the single-hop form); 0 = launch path") \
  X(GP_RES,         gp_res,         BOOL, 1,    ANY,  process, "res_lstm_l and res_lstm_i inside the persistent launches (the residual sums ride the hand-offs); 0 = launch path") \
  X(GP_TAGS,        gp_tags,        BOOL, 1,    ANY,  process, "ring slots tagged with the parity of the ring pass; 0 = slots re-armed with sentinels") \
  X(GP_NRT,         gp_nrt,         BOOL, 1,    ANY,  process, "a padded generator whose real rows fit one 16-row tile skips the padding tile; 0 = both tiles run") \
  X(DP_NRT,         dp_nrt,         BOOL, 1,    ANY,  process, "the same for the discriminator's halves of the fused launches (only together with GP_NRT); 0 = the padding tile runs") \
  X(GP_SCHED,       gp_sched,       INT,  -1,   ANY,  process, "GPersistArgs::sched 0..3: off-chain work of the forward launch behind the lane's publication; -1 = 3 from 64 rows on, else 0") \
  X(GP_DIN0,        gp_din0,        BOOL, 0,    ANY,  process, "layer 0's input gradient inside k_glstm_bwd (built, bit-stable, measured slower)") \
  X(TRAIL_FWD,      trail_fwd,      BOOL, 1,    ANY,  process, "D(G(x)) trailing the generator's forward recurrence in one launch (k_glstm_fwd_dt); 0 = separate launches") \
  X(DFWD_T,         dfwd_t,         BOOL, 0,    ANY,  process, "the discriminator's forward launch in its two-tile form (launch_dlstm_fwd_t) where rows % 32 == 0") \
  X(DHEAD,          dhead,          BOOL, 1,    ANY,  process, "fused discriminator head (logits, LSGAN loss and their gradients in k_dhead); 0 = d_logits + launch_lsgan + GEMMs") \
  X(WGRAD_BATCH,    wgrad_batch,    BOOL, 1,    ANY,  process, "the layers' weight-gradient products as batched launches; 0 = per layer") \
  X(WGRAD_STREAMS,  wgrad_streams,  INT,  2,    ANY,  process, "streams the weight gradients run on: >= 2 puts dWp and the column sums on the side stream (and allows FC_SIDE)") \
  X(FC_SIDE,        fc_side,        BOOL, 1,    ANY,  process, "the FCs' parameter gradients of the G-run on the side stream beside the dK GEMMs (needs WGRAD_STREAMS >= 2)") \
  X(DIN0_SIDE,      din0_side,      BOOL, 0,    ANY,  process, "layer 0's input gradient and what hangs on it on the side stream as well") \
  X(LAZY_SWIZZLE,   lazy_swizzle,   BOOL, 1,    ANY,  process, "fragment-tiled weight copies rebuilt where they are read, not after every update (when every recurrence runs persistent); 0 = after every update") \
  X(FUSED_SEG,      fused_seg,      BOOL, 1,    ANY,  process, "rsrgan_d_step / rsrgan_g_step: the update closes the backward pass's graph segment; 0 = a segment of its own") \
  X(DK_PAD,         dk_pad,         BOOL, 1,    ANY,  process, "kernel gradients of layers whose input width is no multiple of 4 as one stacked product into a padded temporary; 0 = separate products") \
  X(DPIPE_W,        dpipe_w,        INT,  224,  W8,   process, "GEMM workers of the G-run's weight-gradient launches under DPIPE (the rest of the CUs are left to D(real))") \
  X(XCD_GROUPS,     xcd_groups,     BOOL, 1,    ANY,  process, "heavy jobs of a step launch own a group of XCD slots; 0 = every job spans all 8 (the contiguous layout)") \
  X(BP_GROUPS,      bp_groups,      BOOL, 1,    ANY,  process, "the same for the backward step launches' K slices; 0 = no groups") \
  X(GEMM_SELF,      gemm_self,      BOOL, 1,    ANY,  process, "the 256 x 256 / 128 x 256 / 256 x 128 tiles of k_gemm_s among the plans; 0 = leaves them out") \
  X(GEMM_BATCH,     gemm_batch,     INT,  1,    ANY,  process, "batched GEMM launches: 0 = off (one by one), 1 = 192 x 256 tiles of k_gemm_s, 2 = the 128 x 128 form") \
  X(GEMM_BATCH_W,   gemm_batch_w,   INT,  0,    W8,   process, "workers of the 192 x 256 batched launch, leaving the other CUs to the side stream; 0 = all") \
  X(CONV4,          conv4,          INT,  1,    ANY,  process, "4x4x1-MFMA convolution kernels: 0 = never (both directions), 1 = widths that waste 16-wide columns, 2 = every multiple of 4") \
  X(CONV4_KS,       conv4_ks,       INT,  2,    ANY,  process, "their k' split for 512-position workgroups: 4 = two group sets x k' quarters (measured slower), else four x halves") \
  X(WGRAD4,         wgrad4,         INT,  -1,   ANY,  process, "4x4x1-MFMA weight gradient: 0 = never, 1 = widths that are no multiple of 16, 2 = all; -1 = from CONV4 (0 -> 0, else 2)") \
  X(CONV_ROWS,      conv_rows,      BOOL, 1,    ANY,  process, "row-aligned 64-column strips for wide frames, the remaining columns in a second launch; 0 = equal strips") \
  X(WGRAD_DH,       wgrad_dh,       INT,  6,    ANY,  process, "most filter rows per workgroup of k_conv_wgrad for multi-strip frames (3 = the earlier form)") \
  X(BN_NARROW,      bn_narrow,      INT,  4096, MIN0, process, "least row count that takes the narrow batch-norm form (0 = never)") \
  X(BN_SMALL_ROWS,  bn_small_rows,  INT,  384,  ANY,  process, "most rows that take the single-workgroup-per-column-block batch-norm path") \
  X(COLRED_VEC,     colred_vec,     INT,  11,   ANY,  process, "bit m: column-reduction mode m of segan.hip loads 16 bytes per lane (mode 2 stays scalar for parity)") \
  X(RESIDENT_PROBE, resident_probe, BOOL, 1,    ANY,  process, "ask the device whether a persistent launch is resident at once; 0 = trust the CU count") \
  X(RESIDENT_CAP,   resident_cap,   INT,  0,    ANY,  process, "n > 0: the probe's verdict of a device that can hold n workgroups (what a CU mask would make it find)") \
  X(GRAPH_DEBUG,    graph_debug,    BOOL, 0,    ANY,  call,    "report on stderr when the capture of a graph segment fails") \
  X(TRAIL_DBG,      trail_dbg,      INT,  1,    ANY,  call,    "GPersistArgs::dout_trail of a trailing BPTT launch (debugging the hand-off)")
// clang-format on

enum SwKind { SW_BOOL, SW_INT };
enum SwClamp { SW_ANY, SW_MIN0, SW_W8 };

// the one place the environment is read
inline int switch_read(const char* name, SwKind kind, int def, SwClamp clamp) {
  const char* e = getenv(name);
  if (!e) return def;
  const int v = atoi(e);
  if (kind == SW_BOOL) return v != 0;
  if (clamp == SW_MIN0) return v > 0 ? v : 0;
  if (clamp == SW_W8) return v >= 64 && v <= 256 ? (v & ~7) : def;
  return v;
}

#define SW_READ(NAME, kind, def, clamp) switch_read("RSRGAN_" #NAME, SW_##kind, def, SW_##clamp)
// SW_IN_<a>_<b>(x): x where the scopes a and b are the same, else nothing
#define SW_IN_handle_handle(x) x
#define SW_IN_handle_process(x)
#define SW_IN_handle_call(x)
#define SW_IN_process_handle(x)
#define SW_IN_process_process(x) x
#define SW_IN_process_call(x)
#define SW_IN_call_handle(x)
#define SW_IN_call_process(x)
#define SW_IN_call_call(x) x

// constructing one reads its rows
#define X(NAME, field, kind, def, clamp, scope, doc) SW_IN_handle_##scope(const int field = SW_READ(NAME, kind, def, clamp);)
struct HandleSwitches { RSRGAN_SWITCHES(X) };
#undef X
#define X(NAME, field, kind, def, clamp, scope, doc) SW_IN_process_##scope(const int field = SW_READ(NAME, kind, def, clamp);)
struct ProcessSwitches { RSRGAN_SWITCHES(X) };
#undef X
inline const ProcessSwitches& switches() { static const ProcessSwitches s; return s; }
#define X(NAME, field, kind, def, clamp, scope, doc) SW_IN_call_##scope(inline int switch_now_##field() { return SW_READ(NAME, kind, def, clamp); })
RSRGAN_SWITCHES(X)
#undef X

}  // namespace rsr
