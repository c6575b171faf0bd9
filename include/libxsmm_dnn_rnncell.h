/* libxsmm_dnn_rnncell.h -- the RNN cell layer of the reference's DNN interface on the GPU: the forward pass of the five cell
 * types (RNN with ReLU, sigmoid or tanh; LSTM; GRU), and the backward and update passes of all but the GRU (at the end), in fp32, activations in the plain NC format and filters in CK (reference:
 * include/libxsmm_dnn_rnncell.h:37-93, src/libxsmm_dnn_rnncell.c, src/libxsmm_dnn_rnncell_forward.c:218-272,
 * src/libxsmm_dnn_elementwise.c and src/template/libxsmm_dnn_rnncell_st_{rnn,lstm,gru}_fwd_nc_ck_generic.tpl.c with the two LSTM
 * bodies ..._lstm_fwd_nc_kcck_{diffused,fused}.tpl.c). Line numbers below refer to the reference's header unless a file is named.
 *
 * Arithmetic: bit for bit what the reference's generic templates return (the reference run with LIBXSMM_TARGET=hsw), with one
 * reservation that is stated at the end of this paragraph. Tensors: x [max_T][N][C], every other activation [max_T][N][K] -- hp
 * and csp too, of which the cell reads step 0; w [C][G*K] and r [K][G*K] with the gate columns side by side, b [G*K]; G = 4 for LSTM in the order i, c, f, o, 3 for
 * GRU in the order i, c, f, 1 for the simple cells.
 *   Pre-activations. Element (t, n, k) of a gate is one chain acc = fmaf(w or r, x or h, acc) in fp32. It starts from b[k] (LSTM's
 *     f gate: from b_f[k] + forget_bias, one rounded add). It then runs over the segments of the reduction in the order of the
 *     cell (below), inside a segment with the reduction index ascending. The blocks bn, bc and bk play no part in it.
 *   Segment order. BF = 1; if C or K lies in (1024, 2048]: the largest BF <= 8 that divides both C/bc and K/bk; if C or K exceeds
 *     2048: the largest such BF <= 16; C == 2048 and K == 1024: BF = 2 whatever divides. The chunks are (C/bc)/BF blocks of w rows
 *     and (K/bk)/BF blocks of r rows (integer divisions: with the forced BF = 2 a remainder block is not computed, as in the
 *     reference). Simple RNN: all of w, then all of r (no BF). LSTM: all w chunks, then all r chunks -- except C == K == 2048,
 *     where the chunks alternate: w chunk 0, r chunk 0, w chunk 1, ... GRU: always alternating. libxsmm_amd_rnn_segments returns
 *     the list.
 *   sigmoid(v) = 1.0f / (1.0f + (float)exp((double)-v)): exp in double precision, one conversion, a rounded fp32 add and a
 *     correctly rounded fp32 divide. tanh(v) = (float)tanh((double)v). ReLU(v) = (v < 0) ? 0 : v (a NaN and a -0.0 pass).
 *   RNN:  z = the chain over w.x[t] and r.h[t-1] (hp at t = 0), stored in the internal state [T][N][K]; h[t] = act(z).
 *   LSTM: chains over w.x[t], r.h[t-1] for i, ci, f, o; i, f, o = sigmoid, ci = tanh; cs = f * cs[t-1] (csp at t = 0), then
 *         cs = cs + i * ci as a multiply and an add, each rounded; co = tanh(cs); h = o * co. All seven are stored per step.
 *   GRU:  i = sigmoid(chain over w_i.x[t], r_i.h[t-1]); c = sigmoid(chain over w_c.x[t], r_c.h[t-1]); o = h[t-1] * i;
 *         f = tanh(chain over w_f.x[t], r_f.o[t]); h = (1.0f - c) * f, then h = h + c * h[t-1] as a multiply and an add, each
 *         rounded. i, c (INTERNAL_CI), f, o and h are stored per step.
 *   Steps t >= the sequence length are not touched; the tensors keep their max_T strides.
 *   The reservation: exp and tanh are those of the device's double-precision library, which may differ from the host libm's by
 *   a few fp64 ulps; the float results then differ only where the exact value lies that close to a float rounding boundary.
 *
 * Handles (src/libxsmm_dnn_rnncell.c:48-137). datatype_in != datatype_out or a type that is neither F32 nor BF16:
 * _ERR_UNSUPPORTED_DATATYPE; BF16: _ERR_UNSUPPORTED_DATATYPE as well (this engine's own; the reference answers the same below
 * AVX-512); max_T < 1: _ERR_TIME_STEPS_TOO_SMALL. A bn, bc or bk of 0 means 64; a block that does not divide its extent becomes
 * the whole extent with _WARN_RNN_SUBOPTIMAL_{N,C,K}_BLOCKING (the last warning wins, the handle is valid). Layouts (:155-841
 * there) for all 23 RNN tensor types in NC / CK (3 dimensions (C or K, N, T); filters 2: (G*K, C) or (G*K, K), the _TRANS types
 * (C or K, G*K); bias 1) and in NCPACKED / CKPACKED (5 and 4 or 5 dimensions); custom_format is 0; another format gives
 * _ERR_INVALID_FORMAT_GENERAL, another type _ERR_UNKNOWN_TENSOR_TYPE. Scratch and internal-state sizes per cell type and kind are
 * the reference's (:844-962, :1703-1770); bind, get and release check in the reference's order: bind_tensor and release_tensor
 * test the type first (_ERR_UNKNOWN_TENSOR_TYPE), then the handle (and tensor: _ERR_INVALID_HANDLE_TENSOR); get_tensor never
 * writes *status; bind_scratch accepts NULL only for FWD of a simple cell; bind_internalstate of a simple cell refuses NULL with
 * _ERR_SCRATCH_NOT_ALLOCED before it looks at the kind; allocate_forget_bias answers a NULL handle with
 * _ERR_INVALID_HANDLE_TENSOR; set_sequence_length above max_T gives _ERR_RNN_INVALID_SEQ_LEN. A NULL handle where the reference
 * dereferences it (get_scratch_size, bind_scratch) gives _ERR_INVALID_HANDLE. None of these touches a device.
 *
 * execute_st checks, in this order and all before any device is asked for: NULL handle (_ERR_INVALID_HANDLE); a kind other than
 * FWD goes to the backward checks below (ALL and unknown kinds: _ERR_INVALID_KIND); a format pair other than NC / CK
 * (_ERR_INVALID_FORMAT_GENERAL, the reference's status for an unknown pair); an unknown cell type (_ERR_INVALID_RNN_TYPE); an
 * unbound tensor the cell's FWD reads or writes, the internal state of a simple cell among them (_ERR_DATA_NOT_BOUND; the
 * reference dereferences NULL); non-positive N, C, K or threads, or a tensor of 2^31 elements or more (_ERR_GENERAL);
 * tid - start_thread < 0 (_ERR_GENERAL). Then what is this engine's own:
 *   1. The scratch is never read or written and may be host memory: w and r are read where they lie, nothing is reformatted.
 *   2. Threads: a call is complete in itself (the reference's execute_st contains barriers and splits (N/bn)*(K/bk)). The rows
 *      of the minibatch are independent recurrences: logical thread ltid owns the row blocks [ltid*chunk, min((ltid+1)*chunk,
 *      N/bn)), chunk = ceil((N/bn) / desc.threads), and runs all steps and all of K for them. Any subset of the threads, in any
 *      order and on any streams, gives the bits of threads = 1. An empty share or ltid >= threads returns _SUCCESS and launches
 *      nothing.
 *   3. Launches: one per step (GRU: two, o must be complete before f starts), ordered by the stream. Where the order is "all of
 *      w, then all of r", one more launch ahead of them computes bias + w.x for all steps at once (plan "split": T + 1 launches,
 *      GRU 2T + 1); otherwise, or with LIBXSMM_AMD_RNN_PLAN=whole, every step walks the whole list (T, GRU 2T). Both give the
 *      same bits. LIBXSMM_AMD_RNN_PLAN=split is ignored where the order does not allow it.
 *   4. Memory: as for the other layers -- tensors the GPU reaches are processed in place and the call does not wait; a
 *      host-visible tensor makes the call complete on return; pageable host memory is staged, and every staged tensor the pass
 *      writes travels back whole.
 *
 * BWD, UPD and BWDUPD of the simple cells and the LSTM (src/template/libxsmm_dnn_rnncell_st_{rnn,lstm}_bwdupd_nc_ck_generic.tpl.c,
 * ..._lstm_bwdupd_nc_kcck_core.tpl.c without LIBXSMM_RNN_CELL_AVX512), bit for bit like the forward pass and with the same
 * reservation. Every sum of products is one fmaf chain; every elementwise multiply, add and subtraction is rounded on its own.
 *   Simple cells: delta[T-1] = act'(z) * dh; for t < T-1, delta[t][n][k] = dh[t][n][k] continued by the chain over c ascending of
 *     r[k][c] * delta[t+1][n][c], then multiplied by act'(z[t]). act': ReLU (z < 0) ? 0 : 1; sigmoid (1 - s) * s with s as in the
 *     forward pass; tanh 1 - t * t with t = (float)tanh((double)z).
 *   LSTM: dout = dh[T-1], or (+0.0 continued by the chain R^T . [di, dci, df, dp] of step t+1) + dh[t]; then, with dcp starting
 *     from dcs: dcp = dcp + (dout * o) * (1 - co * co); dci = (dcp * i) * (1 - ci * ci); di = (dcp * ci) * (i * (1 - i));
 *     df = (dcp * cs[t-1]) * (f * (1 - f)) (csp at t = 0); dp = (dout * co) * (o * (1 - o)); dcp = f * dcp. GRADIENT_CS_PREV holds
 *     the running dcp and in the end the result; GRADIENT_HIDDEN_STATE_PREV is the chain of step 0 (stored without an add). Both
 *     use step 0 of their tensors and are written by every kind.
 *   Chain order over the G * K filter columns (the LSTM's dx, dout and dhp): for each chunk KB = 0 .. BF-1 the gates i, c, f, o in
 *     turn, each over the K / BF indices of the chunk. BF depends on K alone: 1; for K in (1024, 2048] the largest BF <= 8 that
 *     divides K / bk; above 2048 the largest such BF <= 16. libxsmm_amd_rnn_bwd_segments returns the list.
 *   dx[t][n][c] (BWD, BWDUPD) = +0.0 continued by the chain over the filter columns of w[c][q] * delta[t][n][q]; steps >= the
 *     sequence length are not touched. dw[c][q] and dr[c][q] (UPD, BWDUPD) = +0.0 continued by one chain over the steps descending
 *     and, inside a step, the rows ascending of delta[t][n][q] * x[t][n][c], respectively h[t-1][n][c] (hp at t = 0 -- also with a
 *     single step, where the reference's simple-cell template reads before h). db[q] = +0.0 plus delta[t][n][q] in the same order.
 *   Checks, after the NULL handle and all before any device is asked for: the GRU, ALL and unknown kinds: _ERR_INVALID_KIND; a
 *     handle with no GRADIENT_* tensor bound: _ERR_INVALID_KIND (the answer from before these passes existed; the reference checks
 *     nothing and dereferences NULL); the format pair; then _ERR_DATA_NOT_BOUND for anything the templates read or write under
 *     the kind: r, dh and z (LSTM: csp, cs, i, f, o, ci, co, dcs, dcsp, dhp) always, w and dx for BWD, x, hp, h, dw, dr, db for
 *     UPD; the extents and tid - start_thread < 0 as for FWD (_ERR_GENERAL); a share of more than 65535 * 64 rows (_ERR_GENERAL,
 *     nothing is written).
 *   Threads. BWD divides the rows of the minibatch as FWD does. dw, dr and db sum over all rows and there is no barrier between
 *     calls: with UPD and BWDUPD logical thread 0 launches the whole pass, the others launch nothing and return _SUCCESS.
 *   The deltas of all steps live in [max_T][N][G*K] floats of device memory owned by the handle (allocated by its first backward
 *     call, freed by destroy); the caller's scratch stays unused. Launches: one per step, one for the LSTM's dhp, one for dx per
 *     65535 steps, and three for dw, dr, db -- a function of the sequence length and the kind alone. */
#ifndef LIBXSMM_DNN_RNNCELL_H
#define LIBXSMM_DNN_RNNCELL_H

#include "libxsmm_dnn.h"

/** Opaque handle (:37). */
typedef struct libxsmm_dnn_rnncell libxsmm_dnn_rnncell;

/** The cell types (:40-51). */
typedef enum libxsmm_dnn_rnncell_type {
  LIBXSMM_DNN_RNNCELL_RNN_RELU,    /* simple cell, h = ReLU(z) */
  LIBXSMM_DNN_RNNCELL_RNN_SIGMOID, /* simple cell, h = sigmoid(z) */
  LIBXSMM_DNN_RNNCELL_RNN_TANH,    /* simple cell, h = tanh(z) */
  LIBXSMM_DNN_RNNCELL_LSTM,
  LIBXSMM_DNN_RNNCELL_GRU
} libxsmm_dnn_rnncell_type;

/** The descriptor (:53-67); the order of the fields is the interface. */
typedef struct libxsmm_dnn_rnncell_desc {
  int threads;
  libxsmm_blasint K;     /* outputs */
  libxsmm_blasint N;     /* minibatch */
  libxsmm_blasint C;     /* inputs */
  libxsmm_blasint max_T; /* time steps the tensors are laid out for */
  libxsmm_blasint bk;
  libxsmm_blasint bn;
  libxsmm_blasint bc;
  libxsmm_dnn_rnncell_type cell_type;
  libxsmm_dnn_datatype datatype_in;
  libxsmm_dnn_datatype datatype_out;
  libxsmm_dnn_tensor_format buffer_format; /* activations */
  libxsmm_dnn_tensor_format filter_format; /* w and r */
} libxsmm_dnn_rnncell_desc;

/* :69-70 */
LIBXSMM_API libxsmm_dnn_rnncell* libxsmm_dnn_create_rnncell(libxsmm_dnn_rnncell_desc rnncell_desc, libxsmm_dnn_err_t* status);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_destroy_rnncell(const libxsmm_dnn_rnncell* handle);

/* :72 */
LIBXSMM_API libxsmm_dnn_tensor_datalayout* libxsmm_dnn_rnncell_create_tensor_datalayout(const libxsmm_dnn_rnncell* handle, const libxsmm_dnn_tensor_type type, libxsmm_dnn_err_t* status);

/* :74-77 (get_scratch_ptr returns the address as bound, before alignment) */
LIBXSMM_API size_t libxsmm_dnn_rnncell_get_scratch_size(const libxsmm_dnn_rnncell* handle, const libxsmm_dnn_compute_kind kind, libxsmm_dnn_err_t* status);
LIBXSMM_API void*  libxsmm_dnn_rnncell_get_scratch_ptr (const libxsmm_dnn_rnncell* handle, libxsmm_dnn_err_t* status);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_rnncell_bind_scratch(libxsmm_dnn_rnncell* handle, const libxsmm_dnn_compute_kind kind, const void* scratch);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_rnncell_release_scratch(libxsmm_dnn_rnncell* handle, const libxsmm_dnn_compute_kind kind);

/* :79-82 (the internal state of a simple cell is z, [max_T][N][K] floats; get_internalstate_ptr returns it aligned to 64) */
LIBXSMM_API size_t libxsmm_dnn_rnncell_get_internalstate_size(const libxsmm_dnn_rnncell* handle, const libxsmm_dnn_compute_kind kind, libxsmm_dnn_err_t* status);
LIBXSMM_API void*  libxsmm_dnn_rnncell_get_internalstate_ptr (const libxsmm_dnn_rnncell* handle, libxsmm_dnn_err_t* status);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_rnncell_bind_internalstate(libxsmm_dnn_rnncell* handle, const libxsmm_dnn_compute_kind kind, const void* internalstate);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_rnncell_release_internalstate(libxsmm_dnn_rnncell* handle, const libxsmm_dnn_compute_kind kind);

/* :84-87 */
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_rnncell_allocate_forget_bias(libxsmm_dnn_rnncell* handle, const float forget_bias);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_rnncell_bind_tensor(libxsmm_dnn_rnncell* handle, const libxsmm_dnn_tensor* tensor, const libxsmm_dnn_tensor_type type);
LIBXSMM_API libxsmm_dnn_tensor* libxsmm_dnn_rnncell_get_tensor(libxsmm_dnn_rnncell* handle, const libxsmm_dnn_tensor_type type, libxsmm_dnn_err_t* status);
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_rnncell_release_tensor(libxsmm_dnn_rnncell* handle, const libxsmm_dnn_tensor_type type);

/* :89-90 */
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_rnncell_set_sequence_length(libxsmm_dnn_rnncell* handle, const libxsmm_blasint T);
LIBXSMM_API libxsmm_blasint libxsmm_dnn_rnncell_get_sequence_length(libxsmm_dnn_rnncell* handle, libxsmm_dnn_err_t* status);

/* :92-93 */
LIBXSMM_API libxsmm_dnn_err_t libxsmm_dnn_rnncell_execute_st(libxsmm_dnn_rnncell* handle, libxsmm_dnn_compute_kind kind,
  /*unsigned*/int start_thread, /*unsigned*/int tid);

/** This engine's own, host only: the reduction order of a cell as the list the kernels walk. phase: 0, or 1 for the GRU's f gate
 *  (same list; its r operand is o). Writes up to `capacity` triples (operand pair: 0 = x / w, 1 = h / r; first row of w or r; number
 *  of rows) to `segments` and returns how many the list has (0: bc or bk is not positive or does not divide). */
LIBXSMM_API int libxsmm_amd_rnn_segments(libxsmm_dnn_rnncell_type cell_type, int C, int K, int bc, int bk, int phase, int* segments, int capacity);

/** This engine's own, host only: the order in which the backward passes walk the G * K filter columns (the LSTM's dx, dout and dhp
 *  reductions; a simple cell has one segment of K). Writes up to `capacity` pairs (first column, number of columns) to `segments` and
 *  returns how many the list has (0: bk is not positive or does not divide K, or the cell has no backward pass here). */
LIBXSMM_API int libxsmm_amd_rnn_bwd_segments(libxsmm_dnn_rnncell_type cell_type, int K, int bk, int* segments, int capacity);

#endif /* LIBXSMM_DNN_RNNCELL_H */
