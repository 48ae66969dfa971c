/*
 * quanonet_hea.h -- C ABI of the MI355X-native batched HEA circuit simulator.
 *
 * This is the drop-in boundary for the reference's quantum-layer plug-in
 * (Wang-Ruocheng/QuanONet).  The reference has no C ABI of its own: its boundary
 * is the Python factory `_build_quantum_layer(...) -> nn.Module`
 * (core/models_pt.py:71-100) whose returned module computes
 *     forward(x[B,E]) -> out[B,1]          (core/quantum_circuits_tq.py:65-127)
 * and is differentiated by torch autograd (TorchQuantum) or by MindQuantum's
 * adjoint op `get_expectation_with_grad` (core/quantum_circuits_ms.py:229-233).
 * Each entry point below names the reference interface it replaces.
 *
 * All pointers marked DEVICE are HBM addresses valid on the current HIP device;
 * pointers marked HOST are ordinary host memory read before the call returns.
 * All device work is enqueued on `stream` (a hipStream_t passed as void*; NULL =
 * the null stream).  No entry point allocates, frees or synchronises (except
 * qhea_check_status, whose purpose is to): scratch is the caller-owned `workspace`
 * (size from qhea_workspace_bytes; its first 256 bytes are a header the library
 * maintains -- keep them intact between calls), so every compute call is
 * hipGraph-capturable.  Nothing is retained past return.
 *
 * Layouts (row-major, fp64):
 *   x      [B, E]        encoding angles, column e = block*n + wire, trunk blocks first
 *   w      [blk, 3, n]   ansatz angles: sub-layer, gate (RY,RZ,RY), wire
 *   out    [B]           <psi|H|psi>   (no model bias)
 *   state  [B, 2^n, 2]   final statevector (re,im), basis index little-endian in the wire number
 *   g      [B]           upstream dL/d out_b
 *   grad_x [B, E]        g_b * d out_b / d x[b,e]
 *   grad_w [blk, 3, n]   sum_b g_b * d out_b / d w          (fully reduced, deterministic)
 *
 * Circuit (core/quantum_circuits_tq.py:79-104): start |0..0>; for each block b:
 *   RX(x[:,col]) on wire j%n for j < enc_per_block[b]; then ld_per_block[b] times
 *   { per wire i: RY(w[s,0,i]) RZ(w[s,1,i]) RY(w[s,2,i]);  for i=0..n-1: CNOT(control=(i+1)%n, target=i) }.
 * Read-out (core/quantum_circuits_tq.py:106-127): H = ham_offset + ham_coeff * sum_i P_i, or,
 *   when ham_diag != NULL, H = diag(ham_diag[k]) with bit i of k = wire i.
 *   P is the Pauli named by ham_pauli (QHEA_PAULI_Z/X/Y; generate_simple_hamiltonian's `pauli`,
 *   core/quantum_circuits_ms.py:28-39).  The PyTorch back-ends of the reference only read out Z; X and Y are
 *   the MindQuantum path's --ham_pauli option.  ham_diag requires QHEA_PAULI_Z.
 *
 * Return value: 0 on success, negative QHEA_E* otherwise (qhea_strerror gives text).
 */
#ifndef QUANONET_HEA_H
#define QUANONET_HEA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QHEA_OK            0
#define QHEA_EINVAL       -1   /* bad argument (null pointer, n out of range, ...)   */
#define QHEA_EUNSUPPORTED -2   /* circuit shape not supported by this build           */
#define QHEA_EWORKSPACE   -3   /* workspace too small / missing                       */
#define QHEA_ELAUNCH      -4   /* HIP launch or runtime failure                       */
#define QHEA_ENODEVICE    -5   /* no usable HIP device                                */
#define QHEA_EPIPELINE    -6   /* a backward kernel's wave-to-wave hand-off overran (qhea_check_status) */
#define QHEA_EEXCHANGE    -7   /* a data-parallel exchange did not hear from every rank in time (qhea_dp_status) */

#define QHEA_MIN_QUBITS 2      /* n=1 has no entangler in MindQuantum and an undefined one in TQ */
#define QHEA_MAX_QUBITS 12

/* Library version (major*10000 + minor*100 + patch). */
int qhea_version(void);

/* Text for a QHEA_* code. */
const char* qhea_strerror(int code);

/* Number of usable HIP devices (0 when none); never initialises a context on failure. */
int qhea_device_count(void);

/*
 * Backward-kernel variant for n <= 5 (no reference counterpart; the reference has one autograd path).
 * QHEA_BWD_AUTO (default) chooses by batch density: the psi / lambda / sigma wave pipeline while the sample groups
 * leave SIMDs free, the one-wave-per-group kernel otherwise.  The others force a variant (parity tests, batch sweeps).
 * Process-wide.  The choice fixes the layout of the per-wave partial sums, so set it BEFORE qhea_workspace_bytes()
 * and do not change it while calls that use that workspace are being issued.
 */
#define QHEA_BWD_AUTO   0
#define QHEA_BWD_PACKED 1      /* one wave per sample group: forward sweep, then psi and lambda walked back together */
#define QHEA_BWD_PAIR   2      /* psi wave + lambda wave                                                              */
#define QHEA_BWD_TRI    3      /* psi wave + lambda wave + two inner-product (sigma) waves                            */
#define QHEA_BWD_ZTRI   4      /* the same pipeline on the ZYZ form of the gates with in-kernel (cos, sin) tables     */
                               /* (what AUTO runs for eligible shapes; the values 1-3 also select the first-          */
                               /* generation forward kernel, AUTO, ZTRI and ZPACKED the ZYZ-form one)                 */
#define QHEA_BWD_ZPACKED 5     /* one wave per sample group in the ZYZ form (what AUTO runs once the batch fills the  */
                               /* SIMDs, for circuits whose blocks are one full RX chunk + 1 or 2 sub-layers)         */
#define QHEA_BWD_ZTRI2  6      /* ZTRI with two sample groups per workgroup whose gradient sums are added in LDS: half */
                               /* the partial rows.  AUTO does that only where it costs nothing (batches that fill     */
                               /* every CU's two slots); ZTRI2 forces it from one group per CU on, ZTRI never does it   */
#define QHEA_BWD_ZQUAD  7      /* n = 5, block-unrolled shapes: the pipeline with BOTH sweeps of every chain in the split layout */
                               /* (one sample per chain wave, four chain waves per sample group).  AUTO runs it while every    */
                               /* CU holds at most one sample group; ZQUAD forces it at any batch                               */
#define QHEA_BWD_ZSNAP  8      /* n = 5, block-unrolled shapes, two sample groups per workgroup: one chain wave per sample     */
                               /* sweeps forward storing psi at every publication point, then walks lambda back in the split   */
                               /* layout; the sigma waves read psi from those snapshots (no psi walk back).  AUTO runs it     */
                               /* where it would take ZTRI2 (more sample groups than CUs, at most two per CU; single models, */
                               /* Z / diagonal read-out); ZSNAP forces it at any batch, ZTRI2 forces the psi walk back        */
int qhea_set_backward_variant(int variant);

/*
 * Failure reporting for the pipelined backward kernels (QHEA_BWD_PAIR / QHEA_BWD_TRI).  Their waves hand states to
 * each other through LDS with bounded spins; a wait that overruns its bound aborts the workgroup's pipeline and the
 * kernel ORs a flag into a status word at the start of `workspace`.  The SAME call's reduce kernel then writes NaN
 * into every gradient and into the sse scalar and (qhea_model_train_step) skips the parameter update, so the failure
 * is visible in-band without any host synchronisation.  qhea_check_status() is the explicit check: it copies the
 * status word back on `stream`, WAITS for the stream (the only entry point that synchronises), clears the word and
 * returns QHEA_EPIPELINE if any call since the last check overran, QHEA_OK otherwise (also for a workspace no call has
 * used yet).  Call it where the caller synchronises anyway, e.g. once per epoch.
 */
int qhea_check_status(void* workspace /*DEVICE*/, size_t workspace_bytes, void* stream);

/*
 * Measurement hook (no reference counterpart): the NEXT qhea_backward / qhea_model_loss_grad /
 * qhea_forward / qhea_model_forward call on this thread records `start_event` immediately before and
 * `stop_event` immediately after its circuit kernel (fwd_kernel / bwd_kernel) on the call's stream, then
 * the hook disarms itself.  Both are hipEvent_t handles created with timing enabled; pass NULLs to
 * disarm.  Used by bench.py to time the dominant kernel alone with HIP events.
 */
int qhea_profile_next_circuit_kernel(void* start_event, void* stop_event);

/*
 * Diagnostic (no reference counterpart): n_workgroups one-wave workgroups each time a dependent fp64 FMA chain of `iters`
 * steps with the shader-clock counter and with the constant 100 MHz counter; ticks[2 w] / ticks[2 w + 1] x 100 MHz is the clock
 * workgroup w ran at.  bench.py prints the median, so that a step time can be read against the clock of the device it ran on
 * (devices of one model differ by several percent, and so do the latency-bound kernels here).
 */
int qhea_clock_probe(int n_workgroups, int64_t iters, unsigned long long* ticks /*DEVICE [2 * n_workgroups]*/, void* stream);

/*
 * Bytes of DEVICE scratch the calls below need for this circuit shape and batch.
 * Replaces: nothing in the reference (TorchQuantum allocates per-gate temporaries and
 * autograd saves every intermediate state; core/quantum_circuits_tq.py:74).
 * enc_per_block / ld_per_block: HOST arrays of length n_blocks.
 */
size_t qhea_workspace_bytes(int n_qubits, int n_blocks,
                            const int32_t* enc_per_block, const int32_t* ld_per_block,
                            int64_t batch);

#define QHEA_PAULI_Z 0
#define QHEA_PAULI_X 1
#define QHEA_PAULI_Y 2

/*
 * Forward: out[b] = <psi_b|H|psi_b>.
 * Replaces `_TQHEACircuit.forward` + `_measure` (core/quantum_circuits_tq.py:65-127)
 * and MindQuantum's forward half of `get_expectation_with_grad`
 * (core/quantum_circuits_ms.py:229-233).
 * state_out may be NULL; when given it receives the final statevectors, which
 * qhea_backward can consume to skip its own forward sweep.
 */
int qhea_forward(int n_qubits, int n_blocks,
                 const int32_t* enc_per_block /*HOST*/, const int32_t* ld_per_block /*HOST*/,
                 int64_t batch,
                 const double* x /*DEVICE [B,E]*/, const double* w /*DEVICE [blk,3,n]*/,
                 double ham_offset, double ham_coeff, const double* ham_diag /*DEVICE [2^n] or NULL*/,
                 int ham_pauli /*QHEA_PAULI_**/,
                 double* out /*DEVICE [B]*/, double* state_out /*DEVICE [B,2^n,2] or NULL*/,
                 void* workspace /*DEVICE*/, size_t workspace_bytes, void* stream);

/*
 * Adjoint backward: grad_x, grad_w for upstream g.
 * Replaces torch autograd through the TorchQuantum gate ops
 * (solvers/solver_pt.py:235 `loss.backward()`) and MindQuantum's adjoint gradient
 * (core/quantum_circuits_ms.py:229-233).  O(1) state memory: psi and lambda only.
 * state_in: final statevectors from qhea_forward(state_out) or NULL (recomputed).
 * out may be NULL; when given it receives the forward values as well.
 */
int qhea_backward(int n_qubits, int n_blocks,
                  const int32_t* enc_per_block /*HOST*/, const int32_t* ld_per_block /*HOST*/,
                  int64_t batch,
                  const double* x /*DEVICE [B,E]*/, const double* w /*DEVICE [blk,3,n]*/,
                  double ham_offset, double ham_coeff, const double* ham_diag /*DEVICE or NULL*/,
                  int ham_pauli /*QHEA_PAULI_**/,
                  const double* g /*DEVICE [B]*/, const double* state_in /*DEVICE or NULL*/,
                  double* out /*DEVICE [B] or NULL*/,
                  double* grad_x /*DEVICE [B,E]*/, double* grad_w /*DEVICE [blk,3,n]*/,
                  void* workspace /*DEVICE*/, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Model-level entry points: the same kernels with the reference's classical pre/post-processing and
 * the MSE loss fused in, so that one training step is three launches (prep, circuit, reduce) instead
 * of ~35 framework kernels.  They replace, for the HIP backend,
 *   QuanONetPT.forward / HEAQNNPT.forward            (core/models_pt.py:153-166, 205-213)
 *   _TiledElementWise / _ScaleRepeat                  (core/models_pt.py:14-68)
 *   nn.MSELoss + loss.backward() in the batch loop    (solvers/solver_pt.py:232-236)
 *
 * Parameters travel as ONE flat fp64 DEVICE vector in the order torch's nn.Module.parameters() /
 * state_dict() yields for the reference classes (a module's own parameters before its children's):
 *   QuanONet, trainable_freq=1: [bias (1) | branch_freq.weights (bd*n) | branch_freq.bias (bd*n) |
 *                                trunk_freq.weights (td*n) | trunk_freq.bias (td*n) |
 *                                quantum_layer.ansatz_weights (blk*3*n)]
 *   QuanONet, trainable_freq=0: [bias | quantum_layer.ansatz_weights]
 *   HEAQNN,   trainable_freq=1: [freq.weights (depth*n) | freq.bias (depth*n) | ansatz_weights]
 *   HEAQNN,   trainable_freq=0: [ansatz_weights]
 * and gradients come back in the same layout followed by two scalars [sse, sum_b y_b^2]
 * (grad has qhea_model_param_count()+2 entries) so that a data-parallel caller needs exactly one
 * SUM all-reduce per step.
 * ------------------------------------------------------------------------------------------------ */
#define QHEA_MODEL_QUANONET 0
#define QHEA_MODEL_HEAQNN   1

typedef struct qhea_model_desc {
    int32_t model;            /* QHEA_MODEL_*                                                        */
    int32_t n_qubits;
    int32_t net[4];           /* QuanONet: (branch_depth, branch_ld, trunk_depth, trunk_ld);         */
                              /* HEAQNN:   (depth, linear_depth, 0, 0)                               */
    int32_t branch_in;        /* QuanONet: branch input features; HEAQNN: input features             */
    int32_t trunk_in;         /* QuanONet: trunk input features;  HEAQNN: 0                          */
    int32_t trainable_freq;   /* 1: _TiledElementWise (weights+bias in params); 0: _ScaleRepeat      */
    int32_t ham_pauli;        /* QHEA_PAULI_* read-out basis (0 = Z, the reference's default)          */
    double  scale_coeff;      /* fixed scale when trainable_freq == 0                                */
    double  ham_offset, ham_coeff;   /* H = offset + coeff * sum P_i (ham_diag is passed per call)   */
} qhea_model_desc;

/* Number of trainable scalars for this model (layout above); negative QHEA_E* on a bad descriptor. */
int64_t qhea_model_param_count(const qhea_model_desc* desc);

/* DEVICE scratch bytes for the two calls below. */
size_t qhea_model_workspace_bytes(const qhea_model_desc* desc, int64_t batch);

/*
 * pred[b] = model(branch[b], trunk[b])   (bias included for QuanONet).
 * Replaces QuanONetPT.forward / HEAQNNPT.forward under torch.no_grad()
 * (solvers/solver_pt.py:299-310, infer.py:274-289).  trunk is ignored (may be NULL) for HEAQNN.
 */
int qhea_model_forward(const qhea_model_desc* desc, int64_t batch,
                       const double* branch /*DEVICE [B,branch_in]*/, const double* trunk /*DEVICE [B,trunk_in]*/,
                       const double* params /*DEVICE flat*/, const double* ham_diag /*DEVICE [2^n] or NULL*/,
                       double* pred /*DEVICE [B]*/, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Noisy forward: pred[b] = the model under depolarizing gate noise and readout error, estimated from Monte-Carlo
 * trajectories or from sampled shots; stderr_out[b] (optional) its standard error.  Replaces the deployment half of the
 * reference's ibm_inference.py: `Estimator` with `options.default_shots = S` (shot mode) and, for p1 = p2 = readout = 0,
 * `StatevectorEstimator` (the "Ideal Simulator" line).
 *
 * Noise model (the circuit above; locations in circuit order, which is also the order random numbers are consumed in):
 *   - after each encoding RX, wires 0..n-1: one-qubit depolarizing with probability p1 (X, Y, Z each p1/3);
 *   - after each wire's trainable rotation RY RZ RY (ONE single-qubit gate, as hardware compiles it), wires 0..n-1 of each
 *     sub-layer: the same channel, p1;
 *   - after each CNOT of the ring CNOT(1->0), CNOT(2->1), ..., CNOT(0->n-1): two-qubit depolarizing with probability p2 on
 *     (control, target), each of the 15 non-identity Pauli pairs p2/15;
 *   - readout: every measured bit flips independently with probability q = readout.
 *   A block has n + 2 n ld locations: its n encoding locations, then per sub-layer n rotation locations and n CNOT locations.
 * Estimators:
 *   - expectation mode (shots = 0, trajectories = T >= 1): a trajectory's value is the exact read-out of its final state
 *     with the readout error folded in: H -> offset + coeff (1 - 2q) sum_i P_i, or, with ham_diag,
 *     diag'[k] = sum_j prod_i (bit_i(j) != bit_i(k) ? q : 1 - q) diag[j];  pred = mean over the T trajectories + bias.
 *   - shot mode (shots = S >= 1): every shot is its own trajectory and ends in one bitstring k drawn from |psi|^2 (after a
 *     noiseless basis change for X / Y read-outs: H for X, H S^dagger for Y), then readout flips; the shot's value is
 *     offset + coeff sum_i (1 - 2 b_i), or diag[k] with ham_diag;  pred = mean over the S shots + bias.  (What an Estimator
 *     with default_shots = S estimates for the reference's sum-Z Hamiltonian.)
 *   stderr_out = sample standard deviation of the row's T (or S) values / sqrt(T) (0 for a single value).
 *   p1 = p2 = q = 0 in expectation mode gives the ideal model output.
 * Random numbers: Philox4x32-10, key = (low, high word of seed), counter = (c, trajectory, row_lo, row_hi) with the GLOBAL row
 * index row0 + b, so a row's draws depend on (seed, row, trajectory) only -- not on the batch, the chunking or the launch.
 *   - noise location l uses words 2 (l mod 2) and 2 (l mod 2) + 1 (w0, w1) of call c = floor(l / 2): an error occurs iff
 *     w0 < floor(p 2^32) (64-bit comparison, so p = 1 always fires); the Pauli is (w1 * 3) >> 32 -> X, Y, Z for one qubit,
 *     or k = 1 + ((w1 * 15) >> 32) for two: control Pauli k >> 2, target Pauli k & 3 (0 I, 1 X, 2 Y, 3 Z).
 *   - shot mode, with L = the circuit's location count and m = ceil(L / 2): u = ((a >> 5) 2^26 + (b >> 6)) 2^-53 from words
 *     (0, 1) of call m; the outcome is the first k with u < cdf[k] (|psi_k|^2 accumulated in index order in fp64; if none,
 *     the last k with |psi_k|^2 > 0); bit i (i < n) flips iff word (2 + i) mod 4 of call m + (2 + i) / 4 is < floor(q 2^32).
 * Summation: a row's values are added in a fixed order (trajectories in tiles of 64, slots of 64 / 2^n lanes, then tiles in
 * order; no atomics), so results are bitwise reproducible and the same for any chunking.  Errors are applied as Pauli strings
 * up to a global phase (expectations and sampling probabilities are exactly those of gate-by-gate insertion).
 * Scope: n = 2..6, both models, trainable or fixed frequency, Z / X / Y and ham_diag read-outs.
 * Errors, all before anything is launched: QHEA_EINVAL for p1, p2 or readout outside [0, 1], shots < 0, trajectories < 1 in
 * expectation mode (or more than 2^32 - 1 values per row); QHEA_EUNSUPPORTED for n >= 7.  Launches: the prep kernel, the
 * trajectory kernel, one finishing kernel; no allocation, no synchronisation (hipGraph-capturable).
 */
typedef struct qhea_noise {
    double   p1, p2, readout;   /* depolarizing after each 1q gate / each CNOT; bit-flip per measured bit */
    int64_t  shots;             /* 0: expectation mode; S >= 1: shot mode (one trajectory per shot)    */
    int64_t  trajectories;      /* expectation mode: T >= 1 (ignored in shot mode)                     */
    uint64_t seed;
} qhea_noise;

/* DEVICE scratch bytes for qhea_model_forward_noisy on `batch` rows (0 on a bad descriptor or noise setting). */
size_t qhea_model_noisy_workspace_bytes(const qhea_model_desc* desc, int64_t batch, const qhea_noise* noise);
int    qhea_model_forward_noisy(const qhea_model_desc* desc, int64_t row0, int64_t batch,
                                const double* branch /*DEVICE [B,branch_in]*/, const double* trunk /*DEVICE [B,trunk_in] or NULL*/,
                                const double* params /*DEVICE flat*/, const double* ham_diag /*DEVICE [2^n] or NULL*/,
                                const qhea_noise* noise /*HOST*/,
                                double* pred /*DEVICE [B]*/, double* stderr_out /*DEVICE [B] or NULL*/,
                                void* workspace, size_t workspace_bytes, void* stream);

/*
 * Noisy forward for n = 7..12: the quantity of qhea_model_forward_noisy, word for word -- its noise model, location order,
 * estimators, read-outs, stderr_out and arguments -- for the qubit counts where a state no longer sits one amplitude per lane.
 * Random numbers: unchanged.  Philox4x32-10, counter = (call, trajectory, row_lo, row_hi) with the global row index; the
 * per-location words and the shot-mode words of call m = ceil(L / 2) onward are those stated above (the readout-flip rule
 * reaches call m + 3 at n = 12).
 * Summation, each order a function of n and the number of values per row only:
 *   1. a row's values go in tiles of 64 trajectories; a row's tile sums are added in tile order;
 *   2. inside a tile the trajectories are added in trajectory order;
 *   3. read-out sum_k p_k h(k) (h = the folded read-out, with ham_diag the table diag' built bit by bit,
 *      h <- (1 - q) h + q h[k ^ 2^i] for i = 0..n-1):
 *        n = 7..9:   per lane l (0..63) the terms k = l + 64 r in the order r = 0, 1, ..; then the 64 lane sums by the xor
 *                    butterfly, offsets 32, 16, 8, 4, 2, 1 (lane l adds lane l ^ offset);
 *        n = 10..12: per thread t (0 .. 2^(n-4) - 1) the terms k = 16 t + j in the order j = 0..15; then the butterfly over
 *                    each group of 64 threads, then the groups in order;
 *   4. shot mode, cdf[k] = below(k) + scan(k):
 *        n = 7..9:   blocks of 64 consecutive k; scan = the Hillis-Steele inclusive scan of |psi_k|^2 over the block
 *                    (distances 1, 2, .. 32; position i adds position i - d when i >= d); below = the blocks' totals (scan at
 *                    the block's last position) added in block order from 0;
 *        n = 10..12: chunks of 16 consecutive k; scan = the chunk's running sum in index order; below = the totals of the
 *                    earlier groups of 64 chunks added in order from 0, plus the Hillis-Steele inclusive scan of the chunk totals
 *                    over the group at the chunk before this one (0 for a group's first chunk);
 *      the outcome is the first k with u < cdf[k]; if there is none, the last k with |psi_k|^2 > 0.
 * No floating-point atomics; results are bitwise reproducible and the same for any chunking.
 * Scope: n = 7..12, both models, trainable or fixed frequency, Z / X / Y and ham_diag read-outs.  n <= 6 is QHEA_EUNSUPPORTED:
 * qhea_model_forward_noisy is the implementation for those sizes.  Every other error is the call's above (and QHEA_EINVAL for
 * batch * ceil(values / 64) > 2^31 - 1: a launch has one work item per row and tile), all before anything is launched.  Launches: the prep kernel, (ham_diag in expectation mode: the kernel that builds diag',) the trajectory kernel,
 * the finishing kernel; no allocation, no synchronisation (hipGraph-capturable).
 */
/* DEVICE scratch bytes for qhea_model_forward_noisy_wide on `batch` rows (0 on a bad descriptor or noise setting, or n <= 6). */
size_t qhea_model_noisy_wide_workspace_bytes(const qhea_model_desc* desc, int64_t batch, const qhea_noise* noise);
int    qhea_model_forward_noisy_wide(const qhea_model_desc* desc, int64_t row0, int64_t batch,
                                     const double* branch /*DEVICE [B,branch_in]*/, const double* trunk /*DEVICE [B,trunk_in] or NULL*/,
                                     const double* params /*DEVICE flat*/, const double* ham_diag /*DEVICE [2^n] or NULL*/,
                                     const qhea_noise* noise /*HOST*/,
                                     double* pred /*DEVICE [B]*/, double* stderr_out /*DEVICE [B] or NULL*/,
                                     void* workspace, size_t workspace_bytes, void* stream);

/*
 * Exact noisy forward: the two deterministic quantities the Monte-Carlo call above estimates, computed by carrying the density
 * matrix through the circuit.  The noise model is the one stated for qhea_model_forward_noisy (p1, p2, readout of `noise`;
 * its shots, trajectories and seed are ignored).
 *   pred[b]     = the exact expectation of a read value under those channels + bias: what expectation mode converges to for
 *                 T -> infinity and shot mode for S -> infinity.
 *   shot_std[b] = (optional) the exact standard deviation of ONE shot's value (the read bitstring after its flips ->
 *                 offset + coeff sum_i (1 - 2 b_i), or diag[k] with ham_diag): a row's standard error at S shots is
 *                 shot_std / sqrt(S).  A variance that rounds below zero is returned as zero.
 * Scope: n = 2..6, both models, trainable or fixed frequency, Z / X / Y and ham_diag read-outs.
 * Errors, all before anything is launched and with the outputs untouched: QHEA_EINVAL for p1, p2 or readout outside [0, 1]
 * (NaN included); QHEA_EUNSUPPORTED for n >= 7.  An empty batch returns QHEA_OK.
 * Launches: two -- the prep kernel and the density-matrix kernel (4^n elements per row in LDS, 64 KiB per workgroup); no
 * allocation, no synchronisation (hipGraph-capturable).  No atomics and a fixed summation order: a row's result does not depend
 * on the batch or the chunking (bitwise).  Cost per row: about 2 * 2^n ideal forwards.
 */
/* DEVICE scratch bytes for qhea_model_forward_noisy_exact on `batch` rows (0 on a bad descriptor). */
size_t qhea_model_exact_noisy_workspace_bytes(const qhea_model_desc* desc, int64_t batch);
int    qhea_model_forward_noisy_exact(const qhea_model_desc* desc, int64_t batch,
                                      const double* branch /*DEVICE [B,branch_in]*/, const double* trunk /*DEVICE [B,trunk_in] or NULL*/,
                                      const double* params /*DEVICE flat*/, const double* ham_diag /*DEVICE [2^n] or NULL*/,
                                      const qhea_noise* noise /*HOST: p1, p2, readout used; shots, trajectories, seed ignored*/,
                                      double* pred /*DEVICE [B]*/, double* shot_std /*DEVICE [B] or NULL*/,
                                      void* workspace, size_t workspace_bytes, void* stream);

/*
 * The same two quantities for n = 7..9 (library version 630): qhea_model_forward_noisy_exact with the density matrix in the
 * workspace instead of LDS.  Arguments, noise model (the text of qhea_model_forward_noisy; shots, trajectories and seed are
 * ignored), pred and shot_std are those of the call above.
 * rho of all rows of the call lives in the workspace, 4^n x 16 bytes per row (256 KiB, 1 MiB, 4 MiB for n = 7, 8, 9), element
 * index bit 2q = wire q's row bit, bit 2q + 1 = its column bit.  A stage is one launch of rows x 4^(n-6) workgroups of 256
 * threads; a workgroup copies one tile of 4^6 elements (six wires with both of their bits) into 64 KiB of LDS, runs its passes
 * and copies the tile back.  Stage A holds wires (0..5): element = tile << 12 | local.  Stage B holds wires (0, 1, n-4 .. n-1):
 * element = (local & 15) | tile << 4 | (local >> 4) << (2n - 8).  A sub-layer is stage A (ring passes 0..4) then stage B (ring
 * passes 5..n-1); a block without sub-layers and the basis change of an X / Y read-out are one stage A (wires 0..5) and one
 * stage B (wires 6..n-1).  The launch boundary is the only synchronisation between the tiles of a row: no workgroup waits on
 * another.
 * Launches: the prep kernel, the value-table kernel (h' and h'^2 under the readout confusion, once per call), then
 *   2 * (sub-layers of the circuit) + 2 * (blocks without sub-layers) + (2 for an X or Y read-out)
 * stage launches (one more for a circuit without any block), then the read-out kernel: one wave per row adds p_k h'[k] and
 * p_k h2'[k] over diag rho, lane l the terms k = l + 64 r in the order r = 0, 1, .., then the 64 lane sums by the xor butterfly,
 * offsets 32, 16, 8, 4, 2, 1.  No atomics, no allocation, no synchronisation (hipGraph-capturable); a row's two results are
 * bitwise the same in any call, batch or chunking.
 * Workspace: the tables of the call above, 2 * 2^n doubles, and batch * 4^n * 16 bytes (computed in size_t).
 * Scope: n = 7..9, both models, trainable or fixed frequency, Z / X / Y and ham_diag read-outs, the uniform qhea_noise.  Its
 * counterpart under a qhea_device_noise at these sizes is qhea_model_forward_noisy_device_exact_wide.
 * Errors, all before anything is launched and with the outputs untouched: QHEA_EINVAL for p1, p2 or readout outside [0, 1]
 * (NaN included); QHEA_EUNSUPPORTED for n <= 6 (qhea_model_forward_noisy_exact is the call) and n >= 10; QHEA_EINVAL for
 * batch * 4^(n-6) > 2^31 - 1; QHEA_EWORKSPACE for a short workspace.  An empty batch returns QHEA_OK.
 * Cost: every stage reads and writes rho once, 2 * 4^n * 16 bytes per row; the call is bound by that traffic.
 */
/* DEVICE scratch bytes for qhea_model_forward_noisy_exact_wide on `batch` rows (0 on a bad descriptor, or n outside 7..9). */
size_t qhea_model_exact_noisy_wide_workspace_bytes(const qhea_model_desc* desc, int64_t batch);
int    qhea_model_forward_noisy_exact_wide(const qhea_model_desc* desc, int64_t batch,
                                           const double* branch /*DEVICE [B,branch_in]*/, const double* trunk /*DEVICE [B,trunk_in] or NULL*/,
                                           const double* params /*DEVICE flat*/, const double* ham_diag /*DEVICE [2^n] or NULL*/,
                                           const qhea_noise* noise /*HOST: p1, p2, readout used; shots, trajectories, seed ignored*/,
                                           double* pred /*DEVICE [B]*/, double* shot_std /*DEVICE [B] or NULL*/,
                                           void* workspace, size_t workspace_bytes, void* stream);

/*
 * Noise-aware training: the MSE loss of the exact noisy forward above and its exact gradient, so that a model can be trained
 * with the device's noise in the loss.  Replaces nothing in the reference (its training entry points optimise the ideal
 * circuit; ibm_inference.py reads the device's gate and readout errors only to report them).
 *
 * The quantity.  Noise model: exactly the one stated for qhea_model_forward_noisy (p1 after each encoding RX and after each
 * wire's fused RY RZ RY, p2 after each ring CNOT, the readout flip q folded into the value table h'); shots, trajectories and
 * seed of `noise` are ignored.
 *   pred_b       = what qhea_model_forward_noisy_exact returns for row b (exact noisy expectation + bias);
 *   loss         = sum_b (pred_b - y_b)^2 * inv_batch_total;
 *   grad[0..P)   = d loss / d params in the flat layout of qhea_model_loss_grad;  grad[P] = sum_b (pred_b - y_b)^2;
 *   grad[P+1]    = sum_b y_b^2 -- the [P+2] buffer of the ideal call, so the data-parallel SUM and qhea_adam_step take it as is.
 * The gradient is exact (no sampling, no random numbers): every channel is linear, so the adjoint recipe of qhea_backward
 * carries over with psi -> rho and lambda -> the Heisenberg-picture observable O.  With rho_k the state after operation k and
 * O_k the observable pulled back to that point (O_N = diag h' behind the H / H S^dagger of an X / Y read-out;
 * O_{k-1} = Phi_k^dagger(O_k)):
 *   - a rotation exp(-i theta sigma / 2) on wire q:  d pred / d theta = Im Tr(O_k sigma_q rho_k);  then rho_{k-1} = U^dagger rho_k U,
 *     O_{k-1} = U^dagger O_k U.  The fused RY RZ RY is walked back as its three rotations;
 *   - a depolarizing channel is self-adjoint: O takes the channel itself, rho its inverse (one qubit: off-diagonal pair
 *     / (1 - 4p/3), diagonal pair (keep d0 - mix d1) / (1 - 4p/3); two qubits, lam = 16p/15: unequal-bit elements / (1 - lam),
 *     the four equal-bit ones (x - (lam/4) S) / (1 - lam) with S their sum);  a CNOT is its own inverse on both.
 * Chain rule as in qhea_model_loss_grad: ansatz angles sum over the rows with weight g_b = 2 (pred_b - y_b) inv_batch_total;
 * trainable frequencies: weights[j] += g_b dpred_b/dx_j input_tiled[b, j], bias[j] += g_b dpred_b/dx_j; model bias: sum_b g_b.
 *
 * Conditioning and the guard.  Walking rho back multiplies its traceless part by
 *   A = (1 - 4 p1 / 3)^(-L1) (1 - 16 p2 / 15)^(-L2),   L1 = E + n blk one-qubit locations, L2 = n blk CNOTs,
 * while O shrinks by the same factor, so the traces stay bounded; measured (tests/test_noise_aware_abi.py) the
 * inverse walk agrees with a walk over stored states to 1e-14 for log10 A up to 12 and is still clean at 18.  The calls refuse
 * -- QHEA_EUNSUPPORTED, before anything is launched, outputs untouched -- p1 >= 3/4 or p2 >= 15/16 (a singular channel) and
 * log10 A > 12; qhea_model_exact_noisy_log10_amplification returns log10 A (host only, no device needed; NaN for a bad
 * descriptor or rates outside [0, 1], +inf for a singular channel).  At p1 = 1e-3, p2 = 1e-2 the Q5 Net40-2-20-2 model has
 * log10 A = 3.3.
 *
 * Scope: n = 2..6, both models, trainable or fixed frequency, Z / X / Y and ham_diag read-outs.
 * Errors, all before anything is launched and with the outputs untouched: QHEA_EINVAL for rates outside [0, 1] (NaN included),
 * a NULL noise, a bad descriptor, a negative batch, NULL arrays; QHEA_EUNSUPPORTED for n >= 7 and for the guard;
 * QHEA_EWORKSPACE.  An empty batch (or n_steps = 0) returns QHEA_OK.
 * Launches: three per step -- the prep kernel, the density-matrix backward kernel (rho and O of a row in LDS, 2 x 16 * 4^n
 * bytes; forward sweep, then the reverse walk), one reduce kernel (rows added per parameter, frequency
 * chain rule, and in train_steps the Adam update of qhea_adam_step); no allocation, no synchronisation (hipGraph-capturable).
 * No atomics and fixed summation orders: results are bitwise reproducible, and a row's pred and its d pred / d angle record do
 * not depend on the batch, the grid or the rows beside it.  pred agrees with qhea_model_forward_noisy_exact to rounding (1e-13).
 * qhea_model_train_steps_noisy_exact: arguments and semantics of qhea_model_train_steps with `noise` after ham_diag; bitwise a
 * loop of qhea_model_loss_grad_noisy_exact + qhea_adam_step.  The workspace must fit the largest step.
 */
size_t qhea_model_exact_noisy_grad_workspace_bytes(const qhea_model_desc* desc, int64_t batch);
double qhea_model_exact_noisy_log10_amplification(const qhea_model_desc* desc, const qhea_noise* noise /*HOST*/);
int    qhea_model_loss_grad_noisy_exact(const qhea_model_desc* desc, int64_t batch,
                                        const double* branch, const double* trunk, const double* y /*DEVICE [B]*/,
                                        const double* params, const double* ham_diag,
                                        const qhea_noise* noise /*HOST: p1, p2, readout used*/, double inv_batch_total,
                                        double* grad /*DEVICE [P+2]*/, double* pred /*DEVICE [B] or NULL*/,
                                        void* workspace, size_t workspace_bytes, void* stream);
int    qhea_model_train_steps_noisy_exact(const qhea_model_desc* desc, int64_t n_steps, const int64_t* row_begin /*HOST [n_steps+1]*/,
                                          const double* branch /*DEVICE*/, const double* trunk /*DEVICE or NULL*/,
                                          const double* y /*DEVICE*/, double* params /*DEVICE flat, updated in place*/,
                                          const double* ham_diag, const qhea_noise* noise /*HOST*/,
                                          const double* inv_batch_total /*HOST [n_steps]*/,
                                          double* grad /*DEVICE [n_steps][grad_stride]*/, int64_t grad_stride,
                                          double* exp_avg, double* exp_avg_sq, int64_t first_step, double lr, double beta1,
                                          double beta2, double eps, double weight_decay, void* workspace,
                                          size_t workspace_bytes, void* stream);

/*
 * The same loss and exact gradient for n = 7..9 (library version 650): the quantity, the adjoint walk, the [P+2] buffer and the
 * guard of qhea_model_loss_grad_noisy_exact, with rho and the observable O in the workspace instead of LDS, on the tiles of
 * qhea_model_forward_noisy_exact_wide.  Argument lists: those of the two calls above.
 * rho and O of all rows of the call live in the workspace, 4^n x 16 bytes per row each, in the index layout of the forward.
 * Forward sweep: the value-table kernel, the stage launches and the read-out kernel of qhea_model_forward_noisy_exact_wide;
 * pred_b is bitwise what that call returns for row b.  Then one launch writes O_N = diag(h' - mean h') (zero elsewhere; the
 * identity component carries no gradient), and for an X / Y read-out rho and O go through the daggers of the basis change as
 * one stage B (wires 6..n-1) and one stage A (wires 0..5).  A reverse sub-layer is stage B (ring passes n-1..5) then stage A
 * (ring passes 4..0), each one launch of rows x 4^(n-6) workgroups of 256 threads that hold their tile of rho and their tile of
 * O in 2 x 64 KiB of LDS (one workgroup per CU); a block without sub-layers is one stage B and one stage A.  The tile maps, the
 * local passes and the pending-gate rule are the forward's.
 * Sums: a trace is added over a thread's 16 elements, over the wave by the xor butterfly (offsets 32 .. 1), over the
 * workgroup's four waves in wave order, and written as one partial per (angle, row, tile); the partial buffer holds every angle
 * of the circuit, and ONE fold launch at the end of the walk adds a row's tiles in tile order 0, 1, .. into rec[angle][row] (and
 * copies pred out).  The reduce kernel of qhea_model_loss_grad_noisy_exact then adds the rows (lane l rows l, l + 64, ..; the
 * butterfly) and, in train_steps, applies the Adam update.  No atomics, no flags, no workgroup waits on another; a row's pred
 * and records are bitwise independent of the batch, the grid and the chunking.  qhea_model_train_steps_noisy_exact_wide is
 * bitwise a loop of qhea_model_loss_grad_noisy_exact_wide + qhea_adam_step; its workspace must fit the largest step.
 * Launches per step, with S = sub-layers of the circuit, Z = blocks without sub-layers, R = 1 for an X or Y read-out, else 0:
 *   6 + 4 (S + Z + R)        (prep, value table, 2 (S + Z + R) forward stages, read-out, O_N, 2 R + 2 S + 2 Z reverse stages,
 *                             fold, reduce; one more for a circuit without any block)
 * No allocation, no host synchronisation (hipGraph-capturable).
 * Workspace for `batch` rows, every region rounded up to 256 bytes, computed in size_t, with A = E + 3 n blk angles:
 *   the prep tables of qhea_model_forward_noisy_exact | pred: batch doubles | records: A batch doubles | h', h'^2: 2 * 2^n
 *   doubles | partials: A batch 4^(n-6) doubles | rho: batch 4^n 16 bytes | O: batch 4^n 16 bytes.
 * Scope: n = 7..9, both models, trainable or fixed frequency, Z / X / Y and ham_diag read-outs, the uniform qhea_noise.
 * Errors, all before anything is launched and with the outputs untouched: those of qhea_model_loss_grad_noisy_exact in its
 * order (the guard included: p1 >= 3/4, p2 >= 15/16 or log10 A > 12 is QHEA_EUNSUPPORTED), with QHEA_EUNSUPPORTED for n <= 6
 * (qhea_model_loss_grad_noisy_exact is the call) and n >= 10; then QHEA_EINVAL for batch * 4^(n-6) > 2^31 - 1 (train_steps:
 * the largest step); then QHEA_EWORKSPACE.  An empty batch (or n_steps = 0) returns QHEA_OK.
 * Cost: a forward stage moves rho once each way, a reverse stage rho and O: about three times the traffic of the exact forward.
 */
/* DEVICE scratch bytes for the two calls below on `batch` rows (0 on a bad descriptor, or n outside 7..9). */
size_t qhea_model_exact_noisy_wide_grad_workspace_bytes(const qhea_model_desc* desc, int64_t batch);
int    qhea_model_loss_grad_noisy_exact_wide(const qhea_model_desc* desc, int64_t batch,
                                             const double* branch, const double* trunk, const double* y /*DEVICE [B]*/,
                                             const double* params, const double* ham_diag,
                                             const qhea_noise* noise /*HOST: p1, p2, readout used*/, double inv_batch_total,
                                             double* grad /*DEVICE [P+2]*/, double* pred /*DEVICE [B] or NULL*/,
                                             void* workspace, size_t workspace_bytes, void* stream);
int    qhea_model_train_steps_noisy_exact_wide(const qhea_model_desc* desc, int64_t n_steps, const int64_t* row_begin /*HOST [n_steps+1]*/,
                                               const double* branch /*DEVICE*/, const double* trunk /*DEVICE or NULL*/,
                                               const double* y /*DEVICE*/, double* params /*DEVICE flat, updated in place*/,
                                               const double* ham_diag, const qhea_noise* noise /*HOST*/,
                                               const double* inv_batch_total /*HOST [n_steps]*/,
                                               double* grad /*DEVICE [n_steps][grad_stride]*/, int64_t grad_stride,
                                               double* exp_avg, double* exp_avg_sq, int64_t first_step, double lr, double beta1,
                                               double beta2, double eps, double weight_decay, void* workspace,
                                               size_t workspace_bytes, void* stream);

/*
 * Noise-aware training at n = 7..9, where a density matrix no longer fits: the MSE loss of the SAMPLED noisy forward
 * (qhea_model_forward_noisy_wide, expectation mode) and its gradient with the random stream held fixed.
 *
 * The quantity.  A depolarizing channel is a mixture of Pauli insertions whose probabilities do not depend on the parameters,
 * so for fixed draws a trajectory is an ideal circuit with fixed Pauli strings in it and its value is smooth in the parameters.
 *   pred_b       = what qhea_model_forward_noisy_wide returns for global row row0 + b under the same `noise` (shots = 0, its
 *                  trajectories T and seed): the mean of the T trajectory values + bias.  Agreement is to rounding, not bitwise:
 *                  the summation order below is this call's own;
 *   loss         = sum_b (pred_b - y_b)^2 * inv_batch_total;
 *   grad[0..P)   = the exact derivative of that loss with the random stream held fixed, in the flat layout of
 *                  qhea_model_loss_grad;  grad[P] = sum_b (pred_b - y_b)^2;  grad[P+1] = sum_b y_b^2, as in the exact call.
 * The estimator.  With Var_b the variance of one trajectory's value of row b, the expectation of the sampled loss over the
 * stream is the exact noisy MSE (the loss of qhea_model_loss_grad_noisy_exact) + inv_batch_total sum_b Var_b / T.  Hence
 * d pred_b / d theta is an unbiased estimate of the exact noisy derivative, and the loss gradient is the exact noisy one plus
 * sampling noise plus the derivative of that variance term, which is of order 1 / T.  Nothing is done about the latter: the
 * estimator is stated here, not corrected.
 * The walk.  Per trajectory the forward of qhea_model_forward_noisy_wide, then lambda = h' psi in the read-out basis (h' the
 * folded read-out weight, with ham_diag the table diag'; no residual weight), then the adjoint walk of qhea_backward with the
 * sampled Pauli strings in it (each is its own inverse up to a sign psi and lambda share): per fused RY RZ RY the sums
 * Im<lambda|sigma|psi>, sigma = X, Y, Z, behind the gate; per encoding RX the X sum behind it.
 * Random numbers: exactly those of the forward call -- the same Philox words for the same (seed, global row, trajectory,
 * location).
 * Summation, each order a function of n, the shape and T only:
 *   1. a trajectory's value: as in qhea_model_forward_noisy_wide (3., n = 7..9); its inner products: per lane in register
 *      order, then over the 64 lanes by a fixed transposing butterfly (lane bits 4, 5, 3, 2, 1, 0 for a sub-layer's 3n sums,
 *      0, 1, .. 5 for a block's n encoding sums);
 *   2. a row's trajectories go in tiles of 4; inside a tile values and inner products are added in trajectory order;
 *   3. a row's tiles are added in tile order and divided by T; then a gate's (X, Y, Z) become its three angles' derivatives
 *      (g_c = Y, g_b = cos(c) Z + sin(c) X, g_a = cos(b) Y - sin(b) cos(c) X + sin(b) sin(c) Z for RY(a) RZ(b) RY(c));
 *   4. the rows per parameter as in qhea_model_loss_grad_noisy_exact (lane l adds rows l, l + 64, ..; the 64 lane sums by
 *      the xor butterfly), with the weight 2 (pred_b - y_b) inv_batch_total and the frequency chain rule stated there.
 * qhea_model_train_steps_noisy_wide: arguments and semantics of qhea_model_train_steps_noisy_exact.  Step i has the Adam count
 * t = first_step + i, draws from the stream keyed noise->seed + t (mod 2^64) with global rows row_begin[i] + r, and is bitwise
 * qhea_model_loss_grad_noisy_wide with that seed and row0 = row_begin[i] followed by qhea_adam_step: fresh noise every step,
 * and a run resumed at first_step reproduces an uninterrupted one.  The workspace must fit the largest step.
 * Scope: n = 7..9, both models, trainable or fixed frequency, Z / X / Y and ham_diag read-outs; the uniform model of qhea_noise
 * only (relaxation jumps of a device noise model depend on the state, hence on the parameters).
 * Errors, all before anything is launched and with the outputs untouched, in the order of the forward call: a bad descriptor;
 * QHEA_EINVAL for rates outside [0, 1] (NaN included), a NULL noise, trajectories < 1 and shots > 0 (shot mode has no such
 * gradient); QHEA_EUNSUPPORTED for n <= 6 (the exact calls above) and n >= 10; QHEA_EINVAL for a bad read-out, a negative
 * batch or row0, first_step < 1, NULL arrays, batch * ceil(T / 4) > 2^31 - 1; QHEA_EWORKSPACE.  An empty batch (or
 * n_steps = 0) returns QHEA_OK.  There is no conditioning guard: no channel is inverted.
 * Launches: four per step -- the prep kernel, the trajectory kernel (one wave per row and tile), the fold kernel (tiles -> pred
 * and the per-row record), the reduce kernel of the exact call (with Adam in train_steps) -- and with ham_diag one more per
 * CALL in front, the kernel that builds diag'.  No allocation, no synchronisation (hipGraph-capturable).  No atomics and fixed
 * orders: results are bitwise reproducible, and a row's pred and record do not depend on the batch, the grid or the rows
 * beside it.  Cost per trajectory: one forward walk, two reverse walks and 3 n inner products per sub-layer.
 */
/* DEVICE scratch bytes for the two calls on (at most) `batch` rows (0 on a bad descriptor or noise setting, shots > 0, or n
 * outside 7..9): the forward's tables, and (E + 3 n blk) doubles per (row, tile) and per row. */
size_t qhea_model_noisy_wide_grad_workspace_bytes(const qhea_model_desc* desc, int64_t batch, const qhea_noise* noise);
int    qhea_model_loss_grad_noisy_wide(const qhea_model_desc* desc, int64_t row0, int64_t batch,
                                       const double* branch, const double* trunk, const double* y /*DEVICE [B]*/,
                                       const double* params, const double* ham_diag,
                                       const qhea_noise* noise /*HOST: shots = 0*/, double inv_batch_total,
                                       double* grad /*DEVICE [P+2]*/, double* pred /*DEVICE [B] or NULL*/,
                                       void* workspace, size_t workspace_bytes, void* stream);
int    qhea_model_train_steps_noisy_wide(const qhea_model_desc* desc, int64_t n_steps, const int64_t* row_begin /*HOST [n_steps+1]*/,
                                         const double* branch /*DEVICE*/, const double* trunk /*DEVICE or NULL*/,
                                         const double* y /*DEVICE*/, double* params /*DEVICE flat, updated in place*/,
                                         const double* ham_diag, const qhea_noise* noise /*HOST*/,
                                         const double* inv_batch_total /*HOST [n_steps]*/,
                                         double* grad /*DEVICE [n_steps][grad_stride]*/, int64_t grad_stride,
                                         double* exp_avg, double* exp_avg_sq, int64_t first_step, double lr, double beta1,
                                         double beta2, double eps, double weight_decay, void* workspace,
                                         size_t workspace_bytes, void* stream);

/*
 * The same at n = 10..12, where psi and lambda rest in LDS: quantity, estimator, random stream, record, arguments, launches and
 * error order of the _wide pair above, under names of their own because the _wide pair's answers at n >= 10 are part of its
 * contract.  One workgroup per (row, tile): 2^(n-LG) threads, LG = 3 gate qubits per pass at n = 10 and 11, 4 at n = 12 (128 /
 * 256 / 256 threads), thread t holding in a pass the 2^LG amplitudes that differ in the pass's index bits.
 * Summation, each order a function of n, the shape and T only, so that a row's pred and record depend on (seed, global row, T)
 * and on nothing else -- not on the batch, the grid or the rows beside it:
 *   1. within a thread: a trajectory's value over the thread's 2^LG consecutive basis states 2^LG t + j, j ascending (at
 *      n = 12 the order of qhea_model_forward_noisy_wide, 3.; at n = 10 and 11 groups of 8 where that call has 16); an inner
 *      product over the passes of a reverse layer from the highest index bits down and, inside a pass, over the amplitude pairs
 *      in ascending local index, each pair one chain of fused multiply-adds;
 *   2. over the wave: the value by the xor butterfly (offsets 32, 16, .. 1); the 3n sums of a sub-layer and the n of a block's
 *      encoding by the transposing butterfly of qhea_backward at n = 10..12 (lane bits 0, 1, .. 5);
 *   3. over the waves: in wave order;
 *   4. within a tile of 2 trajectories: values and inner products in trajectory order;
 *   5. over the tiles: in tile order, divided by T, then a gate's (X, Y, Z) to its angles and the rows per parameter exactly as
 *      3. and 4. of the _wide pair.
 * pred agrees with qhea_model_forward_noisy_wide for the same noise and row0 to rounding, not bitwise (other tiles).
 * Scope: n = 10..12; QHEA_EUNSUPPORTED for n <= 9 (the _wide pair and the exact calls), reported where the _wide pair reports its
 * qubit range: after a bad descriptor and a bad noise setting (rates outside [0, 1], NaN, NULL, trajectories < 1, shots > 0),
 * before QHEA_EINVAL for a bad read-out, a negative batch or row0, first_step < 1, NULL arrays and batch * ceil(T / 2) >
 * 2^31 - 1, and before QHEA_EWORKSPACE.  All errors come before anything is launched and leave the outputs untouched.  An empty
 * batch (or n_steps = 0) returns QHEA_OK.  Step i of train_steps has the stream key noise->seed + first_step + i (mod 2^64) and
 * the global rows row_begin[i] + r and is bitwise the single call with that seed and row0 = row_begin[i] followed by
 * qhea_adam_step.  Four launches per step and with ham_diag one more per CALL in front, no allocation, no synchronisation
 * (hipGraph-capturable), no atomics.
 */
/* DEVICE scratch bytes for the two calls on (at most) `batch` rows (0 on a bad descriptor or noise setting, shots > 0, or n
 * outside 10..12): the forward's tables, and (E + 3 n blk) doubles per (row, tile of 2) and per row. */
size_t qhea_model_noisy_lds_grad_workspace_bytes(const qhea_model_desc* desc, int64_t batch, const qhea_noise* noise);
int    qhea_model_loss_grad_noisy_lds(const qhea_model_desc* desc, int64_t row0, int64_t batch,
                                      const double* branch, const double* trunk, const double* y /*DEVICE [B]*/,
                                      const double* params, const double* ham_diag,
                                      const qhea_noise* noise /*HOST: shots = 0*/, double inv_batch_total,
                                      double* grad /*DEVICE [P+2]*/, double* pred /*DEVICE [B] or NULL*/,
                                      void* workspace, size_t workspace_bytes, void* stream);
int    qhea_model_train_steps_noisy_lds(const qhea_model_desc* desc, int64_t n_steps, const int64_t* row_begin /*HOST [n_steps+1]*/,
                                        const double* branch /*DEVICE*/, const double* trunk /*DEVICE or NULL*/,
                                        const double* y /*DEVICE*/, double* params /*DEVICE flat, updated in place*/,
                                        const double* ham_diag, const qhea_noise* noise /*HOST*/,
                                        const double* inv_batch_total /*HOST [n_steps]*/,
                                        double* grad /*DEVICE [n_steps][grad_stride]*/, int64_t grad_stride,
                                        double* exp_avg, double* exp_avg_sq, int64_t first_step, double lr, double beta1,
                                        double beta2, double eps, double weight_decay, void* workspace,
                                        size_t workspace_bytes, void* stream);

/*
 * Exact noisy forward under a calibrated device noise model: pred and shot_std of qhea_model_forward_noisy_exact, with the three
 * numbers of qhea_noise replaced by what a backend's calibration reports -- a gate error per wire and per coupled pair, a
 * readout error per qubit and direction, T1 and T2 per qubit -- and with the time the sequential CNOT ring takes.  Replaces the
 * question the reference's ibm_inference.py profile_hardware prepares (it reads exactly these quantities before a job).
 *
 * Timeline of sub-layer s of a block (all wires of a layer act at once; the ring is sequential):
 *   - if s is the block's first sub-layer: an encoding layer of duration t_rx, RX on every wire;
 *   - a rotation layer of duration t_rot, the fused RY RZ RY on every wire;
 *   - n CNOT slots of duration t_cx each; slot j holds CNOT(control (j+1) mod n -> target j).
 *   A block with linear depth 0 has its encoding layer only.
 * Channels, in this order:
 *   - after a one-qubit gate on wire q: depolarizing with p1[q] (rho -> (1 - p) rho + p/3 sum_P P rho P, as in qhea_noise), then
 *     relaxation of wire q for the layer's duration;
 *   - in slot j: the CNOT, then two-qubit depolarizing with p2[j] on its two wires (each of the 15 non-identity Pauli pairs
 *     p2[j]/15; lam = 16 p2[j] / 15 in the closed form), then relaxation for t_cx on both of its wires;
 *   - if idle != 0: every other wire also relaxes for t_cx in that slot;
 *   - read-out: the noiseless basis change for X / Y as above; then bit q reads 1 given 0 with probability readout01[q] and 0
 *     given 1 with probability readout10[q], independently per bit.
 * Relaxation of wire q for time t is the zero-temperature T1 / T2 channel on that wire's 2 x 2 blocks:
 *     rho01, rho10 <- exp(-t / t2[q]) (rho01, rho10);   z <- exp(-t / t1[q]) z + (1 - exp(-t / t1[q])) tr,
 *   z = rho00 - rho11, tr = rho00 + rho11.  t1 or t2 = +infinity means no decay.  It is not a Pauli channel: it is non-unital and
 *   pulls the wire towards |0>.
 * Closed form.  Every one-wire channel here is phase-covariant, a triple (off, a, b): off-diagonals times `off`, z -> a z + b tr,
 *     rho00' = (1 + a + b)/2 rho00 + (1 - a + b)/2 rho11,   rho11' = (1 - a - b)/2 rho00 + (1 + a - b)/2 rho11.
 *   Depolarizing is (1 - 4p/3, 1 - 4p/3, 0), relaxation (exp(-t/t2), exp(-t/t1), 1 - exp(-t/t1)); "second after first" is
 *   off = off2 off1, a = a2 a1, b = a2 b1 + b2.  Relaxation of one wire commutes with everything on other wires and consecutive
 *   relaxations of one wire add their times, so the model folds exactly into four channel sites per wire (D = depolarizing,
 *   R = relaxation):
 *     site                                              wire 0                       wire q >= 1
 *     0 ENC (after the encoding RX)                     D(p1[0]) then R(t_rx)        D(p1[q]) then R(t_rx)
 *     1 ROT (after the fused rotation)                  D(p1[0]) then R(t_rot)       D(p1[q]) then R(t_rot + (q-1) t_cx)
 *     2 CTL (after the slot where the wire is control)  R(t_cx)                      R(t_cx)
 *     3 TGT (after the slot where the wire is target)   R((n-1) t_cx)                R((n-q) t_cx)
 *   With idle = 0 every CTL and TGT entry is R(t_cx) and ROT carries t_rot only.
 * qhea_device_noise_tables (host only, no device needed) returns that composition: chan[site][q] = (off, a, b) as [4][n][3]
 * doubles and lam2[j] = 16 p2[j] / 15; QHEA_EINVAL for a setting the forward call refuses with it (n = 2..12).  It is
 * deliberately wider than the forward call (n <= 6): the composition is host arithmetic that holds for any ring, and the
 * forward call checks a setting for n = 7..12 with the same code before it answers QHEA_EUNSUPPORTED.
 * qhea_model_forward_noisy_device_exact: arguments, workspace (qhea_model_exact_noisy_workspace_bytes), outputs, launches (two,
 * hipGraph-capturable), determinism (bitwise independent of batch and chunking, no atomics) and cost of
 * qhea_model_forward_noisy_exact.  With p1[q] = p1, p2[j] = p2, readout01 = readout10 = readout, infinite t1 / t2 it computes
 * that call's quantity (to rounding; the channels are evaluated in the triple form), with all rates 0 the ideal model.
 * Scope: n = 2..6, both models, trainable or fixed frequency, Z / X / Y and ham_diag read-outs.  Out of scope: thermal
 * excited-state population, crosstalk, routing (the ring is taken to be native on the chosen wires).  Gradients and training
 * under the model: qhea_model_loss_grad_noisy_device_exact below.
 * Errors, all before anything is launched or any device is touched, outputs untouched: QHEA_EINVAL for a NULL setting or a NULL
 * array in it, n_wires != n, a probability outside [0, 1] or NaN, a duration that is negative, NaN or infinite, t1 or t2 <= 0 or
 * NaN, t2 > 2 t1; then QHEA_EUNSUPPORTED for n >= 7; then the errors of qhea_model_forward_noisy_exact.
 */
typedef struct qhea_device_noise {
    int32_t n_wires, idle;      /* n_wires must equal the model's n; idle != 0: wires outside a slot relax during it */
    const double *p1, *p2, *readout01, *readout10, *t1, *t2;   /* HOST, [n_wires] each; p2[j] belongs to slot j */
    double t_rx, t_rot, t_cx;   /* durations in the unit of t1 / t2 */
} qhea_device_noise;

int qhea_device_noise_tables(int n, const qhea_device_noise* dn /*HOST*/, double* chan /*HOST [4][n][3]*/,
                             double* lam2 /*HOST [n]*/);
int qhea_model_forward_noisy_device_exact(const qhea_model_desc* desc, int64_t batch,
                                          const double* branch /*DEVICE [B,branch_in]*/, const double* trunk /*DEVICE [B,trunk_in] or NULL*/,
                                          const double* params /*DEVICE flat*/, const double* ham_diag /*DEVICE [2^n] or NULL*/,
                                          const qhea_device_noise* dn /*HOST*/,
                                          double* pred /*DEVICE [B]*/, double* shot_std /*DEVICE [B] or NULL*/,
                                          void* workspace, size_t workspace_bytes, void* stream);

/*
 * The same two quantities under the device model for n = 7..9 (library version 640): qhea_model_forward_noisy_device_exact on
 * the tiles of qhea_model_forward_noisy_exact_wide.  Arguments, noise model, pred and shot_std are those of the call above; rho
 * of all rows lives in the workspace, whose layout and size are those of qhea_model_forward_noisy_exact_wide (tiles, stages A
 * and B, copy phases, pending-gate rule and grid are that call's).  Ring pass j applies the pending gates of its wires with their
 * ENC / ROT sites, slot j's CNOT and two-qubit channel, the TGT site of wire j and the CTL site of wire (j + 1) mod n; a
 * stage's local wires are global wires fixed at compile time (stage A: the identity; stage B: local 0, 1 -> 0, 1, local w >= 2
 * -> w + n - 6) and its sites go to it as scalars of the launch.  Relaxation is folded into those sites and adds no launch.
 * Launches: the prep kernel, the value-table kernel (h' and h'^2 under the per-bit asymmetric readout confusion), then
 *   2 * (sub-layers of the circuit) + 2 * (blocks without sub-layers) + (2 for an X or Y read-out)
 * stage launches (one more for a circuit without any block), then the read-out kernel of qhea_model_forward_noisy_exact_wide,
 * its order of summation unchanged.  No atomics, no allocation, no synchronisation (hipGraph-capturable); a row's two results
 * are bitwise the same in any call, batch or chunking.
 * Errors, all before anything is launched and with the outputs untouched: those of qhea_model_forward_noisy_device_exact's
 * setting in its order (QHEA_EINVAL); QHEA_EUNSUPPORTED for n <= 6 (qhea_model_forward_noisy_device_exact is the call) and
 * n >= 10; the errors of qhea_model_forward_noisy_exact; QHEA_EINVAL for batch * 4^(n-6) > 2^31 - 1; QHEA_EWORKSPACE for a
 * short workspace.  An empty batch returns QHEA_OK.
 */
/* DEVICE scratch bytes for qhea_model_forward_noisy_device_exact_wide on `batch` rows (0 on a bad descriptor, or n outside 7..9). */
size_t qhea_model_device_exact_noisy_wide_workspace_bytes(const qhea_model_desc* desc, int64_t batch);
int    qhea_model_forward_noisy_device_exact_wide(const qhea_model_desc* desc, int64_t batch,
                                                  const double* branch /*DEVICE [B,branch_in]*/, const double* trunk /*DEVICE [B,trunk_in] or NULL*/,
                                                  const double* params /*DEVICE flat*/, const double* ham_diag /*DEVICE [2^n] or NULL*/,
                                                  const qhea_device_noise* dn /*HOST*/,
                                                  double* pred /*DEVICE [B]*/, double* shot_std /*DEVICE [B] or NULL*/,
                                                  void* workspace, size_t workspace_bytes, void* stream);

/*
 * Training under the calibrated device noise model: the MSE loss of qhea_model_forward_noisy_device_exact and its exact
 * gradient, so that a model scored under a qhea_device_noise can be trained against it.  Replaces nothing in the reference.
 *
 * The quantity is qhea_model_loss_grad_noisy_exact's with pred_b = what qhea_model_forward_noisy_device_exact returns for row b;
 * the [P+2] buffer has the same layout (gradients, sum_b (pred_b - y_b)^2, sum_b y_b^2), so the data-parallel SUM and
 * qhea_adam_step take it as is, and the chain rule around the circuit is the same.
 *
 * The reverse walk.  It is the walk stated for qhea_model_loss_grad_noisy_exact (d pred / d theta = Im Tr(O_k sigma_q rho_k) at
 * every rotation, rho walked back through inverses, O through Heisenberg adjoints) over the channel sites of the device model.
 * A one-wire site is a phase-covariant triple (off, a, b): off-diagonals times `off`, z -> a z + b tr.
 *   - rho walks back through the inverse, the triple (1 / off, 1 / a, -b / a); it exists whenever off > 0 and a > 0;
 *   - O walks back through the adjoint.  Relaxation is non-unital (b != 0), so this is no longer the channel itself:
 *     off-diagonals times `off`, and on the diagonal pair the TRANSPOSED weight matrix,
 *         O00' = (1 + a + b)/2 O00 + (1 - a - b)/2 O11,     O11' = (1 - a + b)/2 O00 + (1 + a - b)/2 O11;
 *   - the two-qubit depolarizing channel of slot j stays self-adjoint; its inverse is the closed form stated there with the
 *     slot's own lam_j = 16 p2[j] / 15;
 *   - order: slot J applies CNOT, D2(lam_J), the TGT site of wire J, the CTL site of wire J + 1 mod n, so the reverse pass undoes
 *     the two one-wire sites first, then D2, then the CNOT (the sites do not commute with D2 once b != 0); a wire's pending
 *     gates are followed by their ENC / ROT site, so in reverse: the site's inverse on rho and adjoint on O, then the trace,
 *     then the un-rotation;
 *   - read-out: O_N = diag h' behind the H / H S^dagger of an X / Y read-out, h' mixed per bit by readout01 / readout10 as in
 *     the forward call.
 *
 * Conditioning and the guard.  With the sums over what the circuit applies -- the ENC site of a wire once per encoding layer,
 * its ROT, CTL and TGT sites once per sub-layer, every CNOT slot once per sub-layer --
 *     log10 A_dev = - sum log10 min(off, a) - sum log10 (1 - lam_j).
 * For p1[q] = p1, p2[j] = p2 and no relaxation this is log10 A of qhea_model_exact_noisy_log10_amplification.
 * qhea_model_device_noisy_log10_amplification returns it (host only, no device needed; NaN for a bad descriptor or a setting the
 * forward call refuses with QHEA_EINVAL, +inf for a singular channel).  The calls refuse -- QHEA_EUNSUPPORTED, before anything
 * is launched, outputs untouched -- p1[q] >= 3/4, p2[j] >= 15/16, a site the circuit applies whose min(off, a) is 0 (a decay
 * that underflows), n >= 7, and log10 A_dev > 7.
 *   The bound is 7, not the uniform call's 12.  Once b != 0 the observable no longer shrinks by the factor rho grows by, and
 *   the numpy probe (tests/test_device_noise_training_abi.py: inverse walk against a walk over stored forward states, device
 *   settings with relaxation on every wire but one; n = 5 with 60 and 120 sub-layers, n = 6 with 20; the largest difference of
 *   the three circuits) shows
 *       log10 A_dev      0        4        5        6        7        8        10       11.99
 *       difference    6.1e-15  2.1e-15  1.3e-14  4.5e-14  2.4e-13  1.5e-12  3.7e-11  1.1e-9
 *   The criterion is the uniform bound's -- no probe at or below the bound above 1e-12 -- and 7 is the largest probed value that
 *   meets it.
 *
 * Scope: n = 2..6, both models, trainable or fixed frequency, Z / X / Y and ham_diag read-outs.
 * Arguments: those of qhea_model_loss_grad_noisy_exact / qhea_model_train_steps_noisy_exact with `dn` in place of `noise`.
 * Workspace: qhea_model_device_noisy_grad_workspace_bytes (0 on a bad descriptor): the uniform call's plus the table below.
 * Errors, all before anything is launched and with the outputs untouched, in this order: a bad descriptor and the setting's
 * QHEA_EINVAL cases (those of qhea_model_forward_noisy_device_exact, by the same code); QHEA_EUNSUPPORTED for n >= 7 and for
 * the guard; then the errors of qhea_model_loss_grad_noisy_exact (read-out, negative batch, NULL arrays, QHEA_EWORKSPACE).
 * An empty batch (or n_steps = 0) returns QHEA_OK.
 * Launches: a table kernel once per call (one workgroup: the three forms -- forward, inverse, adjoint -- of every site, the
 * slots' factors and the readout probabilities, 66 doubles per wire, from its by-value argument into the workspace; the
 * backward kernel reads a site's constants where it uses them), then three per step: the prep kernel, the density-matrix
 * backward kernel (density_dev_bwd_kernel: layout, passes, LDS budget and trace sums of the uniform call's kernel) and that
 * call's reduce kernel.  No allocation, no synchronisation (hipGraph-capturable), no atomics, fixed summation orders: results
 * are bitwise reproducible, and a row's pred and its record do not depend on the batch, the grid or the rows beside it.  pred
 * agrees with qhea_model_forward_noisy_device_exact to rounding (1e-13).
 * qhea_model_train_steps_noisy_device_exact is bitwise a loop of qhea_model_loss_grad_noisy_device_exact + qhea_adam_step.  The
 * workspace must fit the largest step.
 */
size_t qhea_model_device_noisy_grad_workspace_bytes(const qhea_model_desc* desc, int64_t batch);
double qhea_model_device_noisy_log10_amplification(const qhea_model_desc* desc, const qhea_device_noise* dn /*HOST*/);
int    qhea_model_loss_grad_noisy_device_exact(const qhea_model_desc* desc, int64_t batch,
                                               const double* branch, const double* trunk, const double* y /*DEVICE [B]*/,
                                               const double* params, const double* ham_diag,
                                               const qhea_device_noise* dn /*HOST*/, double inv_batch_total,
                                               double* grad /*DEVICE [P+2]*/, double* pred /*DEVICE [B] or NULL*/,
                                               void* workspace, size_t workspace_bytes, void* stream);
int    qhea_model_train_steps_noisy_device_exact(const qhea_model_desc* desc, int64_t n_steps,
                                                 const int64_t* row_begin /*HOST [n_steps+1]*/,
                                                 const double* branch /*DEVICE*/, const double* trunk /*DEVICE or NULL*/,
                                                 const double* y /*DEVICE*/, double* params /*DEVICE flat, updated in place*/,
                                                 const double* ham_diag, const qhea_device_noise* dn /*HOST*/,
                                                 const double* inv_batch_total /*HOST [n_steps]*/,
                                                 double* grad /*DEVICE [n_steps][grad_stride]*/, int64_t grad_stride,
                                                 double* exp_avg, double* exp_avg_sq, int64_t first_step, double lr, double beta1,
                                                 double beta2, double eps, double weight_decay, void* workspace,
                                                 size_t workspace_bytes, void* stream);

/*
 * The same two calls past the guard: rho replayed from stored states (library version 620).
 *
 * qhea_model_loss_grad_noisy_device_exact_stored / qhea_model_train_steps_noisy_device_exact_stored compute what the two calls
 * above compute -- same arguments, same [P+2] buffer, same status codes in the same order -- for settings whose log10 A_dev is
 * past 7.  Call one sub-layer a unit (a block's first sub-layer carries the block's encoding gates; a block without sub-layers
 * is one encoding-only unit), U = sub-layers + blocks without sub-layers.  The forward sweep of the backward kernel writes the
 * row's rho after unit u to snap[u][row] in the workspace (16 * 4^n bytes, fp64 complex, not compressed); the reverse walk
 * replaces rho by the stored rho_u before it undoes unit u.  Within a unit nothing differs from the walk above: rho through
 * the inverse sites and un-rotations, O through the adjoints, the traces where they are.  So rho never carries more than one
 * unit's worth of inverse walk, and the guard is asked of one unit:
 *     qhea_model_device_noisy_log10_layer_amplification (host only) = log10 A_dev of the largest single unit: one sub-layer's
 *     ROT, CTL and TGT sites and CNOT slots, plus the ENC sites once if the circuit has encoding layers; the ENC sites alone
 *     for a circuit without sub-layers.  NaN and +inf exactly where qhea_model_device_noisy_log10_amplification returns them;
 *     never above it, and equal to it for a circuit of one unit.
 * The calls refuse -- QHEA_EUNSUPPORTED, before anything is launched, outputs untouched, at the place in the order where the
 * calls above refuse -- n >= 7, a singular channel (+inf), and a layer amplification above 7: the bound above was measured for
 * the inverse walk of a whole circuit, and one unit is such a circuit.  The total log10 A_dev is no reason to refuse.
 * Workspace: qhea_model_device_noisy_stored_grad_workspace_bytes = qhea_model_device_noisy_grad_workspace_bytes plus the
 * snapshot region behind it, U * batch * 16 * 4^n bytes rounded up to 256 (it passes 4 GiB at sizes people run: Q6 with 20
 * units at 3300 rows; every index is 64-bit).
 * Launches: those of the calls above with density_dev_stored_bwd_kernel in place of density_dev_bwd_kernel; the snapshot of a
 * unit is the row's image in LDS, stored and loaded by the same thread with 16-byte vector accesses (the load is issued one
 * unit ahead and waits in registers), a tail slot of the last workgroup stores and loads none.  No allocation, no synchronisation, no atomics, fixed summation orders: bitwise reproducible,
 * a row's pred and record independent of batch and grid; pred is the same sweep's as above (it agrees to 1e-13).
 * qhea_model_train_steps_noisy_device_exact_stored is bitwise a loop of the loss_grad call + qhea_adam_step.
 */
size_t qhea_model_device_noisy_stored_grad_workspace_bytes(const qhea_model_desc* desc, int64_t batch);
double qhea_model_device_noisy_log10_layer_amplification(const qhea_model_desc* desc, const qhea_device_noise* dn /*HOST*/);
int    qhea_model_loss_grad_noisy_device_exact_stored(const qhea_model_desc* desc, int64_t batch,
                                                      const double* branch, const double* trunk, const double* y /*DEVICE [B]*/,
                                                      const double* params, const double* ham_diag,
                                                      const qhea_device_noise* dn /*HOST*/, double inv_batch_total,
                                                      double* grad /*DEVICE [P+2]*/, double* pred /*DEVICE [B] or NULL*/,
                                                      void* workspace, size_t workspace_bytes, void* stream);
int    qhea_model_train_steps_noisy_device_exact_stored(const qhea_model_desc* desc, int64_t n_steps,
                                                        const int64_t* row_begin /*HOST [n_steps+1]*/,
                                                        const double* branch /*DEVICE*/, const double* trunk /*DEVICE or NULL*/,
                                                        const double* y /*DEVICE*/, double* params /*DEVICE flat, updated in place*/,
                                                        const double* ham_diag, const qhea_device_noise* dn /*HOST*/,
                                                        const double* inv_batch_total /*HOST [n_steps]*/,
                                                        double* grad /*DEVICE [n_steps][grad_stride]*/, int64_t grad_stride,
                                                        double* exp_avg, double* exp_avg_sq, int64_t first_step, double lr,
                                                        double beta1, double beta2, double eps, double weight_decay,
                                                        void* workspace, size_t workspace_bytes, void* stream);

/*
 * The same loss and exact gradient for n = 7..9 (library version 660): the quantity, the inverse walk, the [P+2] buffer and the
 * arguments of qhea_model_loss_grad_noisy_device_exact / qhea_model_train_steps_noisy_device_exact, on the tiles of
 * qhea_model_loss_grad_noisy_exact_wide.  pred is the prediction of qhea_model_forward_noisy_device_exact_wide, bitwise: the
 * forward sweep is that call's launch sequence (same value-table, stage and read-out kernels).
 *
 * rho and O of all rows live in the workspace.  After the forward sweep one launch writes O = diag(h' - mean h') with h' from
 * the asymmetric readout; an X / Y read-out takes rho and O through the daggers of the basis change (two launches, no noise).
 * A reverse sub-layer is two launches over rows * 4^(n-6) workgroups of 256 threads with the tiles of rho and O in 2 x 64 KiB
 * of LDS: stage B with the ring passes j = n-1..5, then stage A with j = 4..0.  Per pass, in global wires: the TGT site of
 * wire j and the CTL site of wire (j + 1) mod n (inverse form on rho, adjoint form on O), D2 of slot j (the slot's inverse on
 * rho, its forward factors on O) with the CNOT, then per pending wire (pass 0: wire 0; every pass j <= n-2: wire j + 1) the
 * ROT site, the three traces with their un-rotations, and in a block's first sub-layer the ENC site, its trace and RX^dagger.
 * A block without sub-layers is two launches, wires 6..n-1 then 0..5: ENC site, trace, RX^dagger.  Traces are written as one
 * partial per (angle, row, tile) and folded in tile order by one launch at the end, as in the uniform call.
 * Constants: a table of [stage][local wire] records (the 66-double record of the n <= 6 call; the forward form and the readout
 * entries stay zero) holds the inverse and adjoint form of every site and the four D2 factors of every slot at the local index
 * the pass uses; one table kernel per call (one workgroup) places what the host composed per global wire; the reverse stages
 * read a site's constants where they use them.
 *
 * Guard: qhea_model_device_noisy_log10_amplification (it answers at every n = 2..12) must be <= 7, the bound of the n <= 6
 * call: the numpy probe of tests/test_device_exact_noisy_wide_training_abi.py (inverse against stored walk, n = 7 with 20
 * sub-layers, n = 8 with 10) shows 9.8e-15 and 6.2e-15 at 7, 6.7e-14 and 3.1e-14 at 8.
 * Errors, all before anything is launched and with the outputs untouched, in this order: a bad descriptor and the setting's
 * QHEA_EINVAL cases; QHEA_EUNSUPPORTED for n outside 7..9 and for the guard (a singular channel, p1 >= 3/4, p2 >= 15/16 are
 * +inf); then the errors of qhea_model_loss_grad_noisy_exact (read-out, negative batch, NULL arrays); QHEA_EINVAL for a batch
 * (or a largest step) above INT_MAX >> 2 (n - 6); QHEA_EWORKSPACE.  train_steps reports first_step < 1 where
 * qhea_model_train_steps_noisy_device_exact reports it (after these checks' QHEA_EINVAL / QHEA_EUNSUPPORTED cases, before the
 * return of a call without steps).  An empty batch (or n_steps = 0) returns QHEA_OK.
 * Workspace: qhea_model_device_noisy_wide_grad_workspace_bytes (0 for a bad descriptor, batch < 0 or n outside 7..9):
 * qhea_model_exact_noisy_wide_grad_workspace_bytes for the largest step plus the table, 2 * 6 * 66 doubles rounded up to 256
 * bytes.
 * Launches per step: 6 + 4 (S + Z + R), S sub-layers, Z blocks without sub-layers, R = 1 for an X / Y read-out (one more for
 * a circuit without blocks), plus the table kernel once per call.  No allocation, no synchronisation (hipGraph-capturable, one
 * linear chain), no atomics, fixed summation orders: bitwise reproducible, a row's pred and records independent of the batch,
 * the grid and the chunking.  qhea_model_train_steps_noisy_device_exact_wide is bitwise a loop of
 * qhea_model_loss_grad_noisy_device_exact_wide + qhea_adam_step; its workspace must fit the largest step.
 */
size_t qhea_model_device_noisy_wide_grad_workspace_bytes(const qhea_model_desc* desc, int64_t batch);
int    qhea_model_loss_grad_noisy_device_exact_wide(const qhea_model_desc* desc, int64_t batch,
                                                    const double* branch, const double* trunk, const double* y /*DEVICE [B]*/,
                                                    const double* params, const double* ham_diag,
                                                    const qhea_device_noise* dn /*HOST*/, double inv_batch_total,
                                                    double* grad /*DEVICE [P+2]*/, double* pred /*DEVICE [B] or NULL*/,
                                                    void* workspace, size_t workspace_bytes, void* stream);
int    qhea_model_train_steps_noisy_device_exact_wide(const qhea_model_desc* desc, int64_t n_steps,
                                                      const int64_t* row_begin /*HOST [n_steps+1]*/,
                                                      const double* branch /*DEVICE*/, const double* trunk /*DEVICE or NULL*/,
                                                      const double* y /*DEVICE*/, double* params /*DEVICE flat, updated in place*/,
                                                      const double* ham_diag, const qhea_device_noise* dn /*HOST*/,
                                                      const double* inv_batch_total /*HOST [n_steps]*/,
                                                      double* grad /*DEVICE [n_steps][grad_stride]*/, int64_t grad_stride,
                                                      double* exp_avg, double* exp_avg_sq, int64_t first_step, double lr,
                                                      double beta1, double beta2, double eps, double weight_decay,
                                                      void* workspace, size_t workspace_bytes, void* stream);

/*
 * The same two calls past the guard: rho replayed from stored states on tiles (library version 670).
 *
 * qhea_model_loss_grad_noisy_device_exact_wide_stored / qhea_model_train_steps_noisy_device_exact_wide_stored compute what the
 * two calls above compute -- same arguments, same [P+2] buffer, n = 7..9 -- for settings whose log10 A_dev is past 7, the way
 * the _stored calls of version 620 do for n <= 6.  A unit is one sub-layer (a block's first sub-layer carries the block's
 * encoding gates) or the encoding of a block without sub-layers; U = sub-layers + blocks without sub-layers.  snap[u] holds
 * every row's rho after unit u, row r at element (u * batch + r) * 4^n (64-bit arithmetic), behind the regions of the calls
 * above.
 * Forward sweep: the launch sequence above with the same value-table, stage B and read-out kernels; stage A of unit u is the
 * same stage loading the row from snap[u-1] (u = 0: nothing) and storing it to snap[u], stage B of unit u works in place on
 * snap[u].  Stage A of an X / Y basis change loads snap[U-1] and stores to the running rho buffer of the calls above, so the
 * last snapshot stays; the read-out kernel reads that buffer (X / Y) or snap[U-1] (Z).  The arithmetic is untouched: pred is
 * bitwise that of the calls above and of qhea_model_forward_noisy_device_exact_wide.
 * Reverse walk: the reverse stages above -- same passes, same table, same trace partials, fold and reduce.  Stage B of unit u
 * loads its rho tile from snap[u] and stores it to the running buffer (the snapshots are read-only after the forward sweep);
 * stage A loads what stage B stored and stores no rho: the next unit starts from snap[u-1].  O is walked in place as above, and
 * the daggers of the basis change are applied as above.  A circuit without blocks has U = 0, takes no snapshot and runs the
 * launches of the calls above.
 * Guard: rho never carries more than one unit's worth of inverse walk, so the bound is asked of one unit:
 * qhea_model_device_noisy_log10_layer_amplification (it answers at every n = 2..12) must be <= 7 -- the bound above, measured
 * on whole circuits, of which one unit is one.  The total log10 A_dev is no reason to refuse.
 * Errors, all before anything is launched and with the outputs untouched, in the order of the calls above: a bad descriptor
 * and the setting's QHEA_EINVAL cases; QHEA_EUNSUPPORTED for n outside 7..9, then for a layer amplification above 7 (a singular
 * channel is +inf); the shared errors; QHEA_EINVAL for a batch (or a largest step) above INT_MAX >> 2 (n - 6);
 * QHEA_EWORKSPACE.  train_steps reports first_step < 1 where the call above reports it.  The _stored calls of version 620
 * keep refusing n >= 7, and the calls above keep their guard on the total.
 * Workspace: qhea_model_device_noisy_wide_stored_grad_workspace_bytes (0 for a bad descriptor, batch < 0 or n outside 7..9) =
 * qhea_model_device_noisy_wide_grad_workspace_bytes + U * batch * 16 * 4^n rounded up to 256 bytes: 4 MiB per row and unit at
 * n = 9 (Net20-2-10-2, 60 units: 240 MiB per row), so the region passes 4 GiB at sizes people run.
 * Launches per step: 6 + 4 (S + Z + R) as above, S sub-layers, Z blocks without sub-layers, R = 1 for an X / Y read-out, plus
 * the table kernel once per call: 1 prep, 1 value table, 2 (S + Z + R) forward stages, 1 read-out, 1 O_N, 2 R daggers,
 * 2 (S + Z) reverse stages, 1 fold, 1 reduce.  By byte count (an estimate) a step moves no more than the call above and one rho store
 * per unit less.  No allocation, no synchronisation (hipGraph-capturable, one linear chain), no atomics, fixed summation orders:
 * bitwise reproducible, a row's pred and records independent of the batch, the grid and the chunking.
 * qhea_model_train_steps_noisy_device_exact_wide_stored is bitwise a loop of the loss_grad call + qhea_adam_step; its workspace
 * must fit the largest step.
 */
size_t qhea_model_device_noisy_wide_stored_grad_workspace_bytes(const qhea_model_desc* desc, int64_t batch);
int    qhea_model_loss_grad_noisy_device_exact_wide_stored(const qhea_model_desc* desc, int64_t batch,
                                                           const double* branch, const double* trunk,
                                                           const double* y /*DEVICE [B]*/, const double* params,
                                                           const double* ham_diag, const qhea_device_noise* dn /*HOST*/,
                                                           double inv_batch_total, double* grad /*DEVICE [P+2]*/,
                                                           double* pred /*DEVICE [B] or NULL*/, void* workspace,
                                                           size_t workspace_bytes, void* stream);
int    qhea_model_train_steps_noisy_device_exact_wide_stored(const qhea_model_desc* desc, int64_t n_steps,
                                                             const int64_t* row_begin /*HOST [n_steps+1]*/,
                                                             const double* branch /*DEVICE*/, const double* trunk /*DEVICE or NULL*/,
                                                             const double* y /*DEVICE*/,
                                                             double* params /*DEVICE flat, updated in place*/,
                                                             const double* ham_diag, const qhea_device_noise* dn /*HOST*/,
                                                             const double* inv_batch_total /*HOST [n_steps]*/,
                                                             double* grad /*DEVICE [n_steps][grad_stride]*/, int64_t grad_stride,
                                                             double* exp_avg, double* exp_avg_sq, int64_t first_step, double lr,
                                                             double beta1, double beta2, double eps, double weight_decay,
                                                             void* workspace, size_t workspace_bytes, void* stream);

/*
 * Noisy forward under the calibrated device noise model by quantum-jump (Monte-Carlo wave-function) trajectories: an unbiased
 * estimate of pred of qhea_model_forward_noisy_device_exact, for the qubit counts that call cannot reach (n = 7..9) and for
 * finite shots at any n = 2..9 -- what an Estimator with default_shots = S returns on that device.  Arguments, estimators and
 * stderr_out are those of qhea_model_forward_noisy with the noise setting split in two: `dn` (the device) and `sampling`.
 *
 * Model.  Exactly the qhea_device_noise model above, timeline and the four folded sites per wire included.  Folding the idle
 * slots into the sites is exact as a channel, so a trajectory sees one relaxation R(tau) per site with the folded duration:
 *   ENC t_rx;  ROT t_rot, or t_rot + (q - 1) t_cx for q >= 1 with idle;  CTL t_cx;  TGT (n - 1) t_cx for wire 0 and
 *   (n - q) t_cx for q >= 1;  with idle = 0: t_cx for CTL and TGT, t_rot for ROT.
 * Unravelling of R(tau) on wire q:  gamma = 1 - exp(-tau / t1[q]);  f = exp(-tau / t2[q]) / sqrt(1 - gamma), clipped to <= 1,
 *   f = 0 when gamma = 1;  pz = (1 - f) / 2.  Two events, in this order:
 *     1. dephasing: Z on wire q with probability pz (state-independent);
 *     2. damping: with P1 the population of wire q in |1> of the current normalised state, with probability gamma P1 the state
 *        becomes |0><1|_q psi / sqrt(P1), otherwise diag(1, sqrt(1 - gamma))_q psi / sqrt(1 - gamma P1).
 *   An infinite t1 or a zero duration gives gamma = 0 and the damping event is the identity, bit for bit.  (Amplitude damping
 *   followed by phase damping: the Kraus pair of the exact call's relaxation.)  Depolarizing stays the sampled Pauli of
 *   qhea_noise, with p1[q] per wire and p2[j] per slot.  qhea_device_noise_jump_tables (host only, no device needed, n = 2..12
 *   like qhea_device_noise_tables) returns jump[site][q] = (gamma, pz) as [4][n][2] doubles.
 * Events in circuit order, which is also the order random numbers are consumed in:
 *   - per block: for q = 0..n-1 the encoding RX on q, then site ENC_q;
 *   - per sub-layer: for q = 0..n-1 the fused rotation on q, then site ROT_q; then for j = 0..n-1: CNOT((j+1) mod n -> j), the
 *     pair Pauli with p2[j], relaxation TGT of wire j, relaxation CTL of wire (j+1) mod n.
 *   A site ENC_q or ROT_q is: Pauli with p1[q], then dephasing, then damping.
 * Random numbers: Philox4x32-10, key = seed, counter = (call, trajectory, row_lo, row_hi) with the GLOBAL row index row0 + b.
 *   Every event group is one whole call: words 0 and 1 pick the Pauli by the rule of qhea_noise (error iff w0 < floor(p 2^32);
 *   one qubit (w1 * 3) >> 32, two qubits 1 + ((w1 * 15) >> 32) with control = code >> 2, target = code & 3); word 2 is the
 *   dephasing, Z iff w2 < floor(pz 2^32); word 3 is the damping, which jumps iff (w3 + 0.5) 2^-32 < gamma P1 in fp64.  The
 *   kernels carry the state unnormalised with its squared norm N2 beside it and evaluate that as u N2 < gamma M, M the masked
 *   sum below (P1 = M / N2; a jump leaves N2 = M, no jump N2 - gamma M); a replay that normalises at every site agrees except
 *   where u lies within a few ulps of the edge.
 *   ENC_q and ROT_q take one call each; slot j takes two: the first gives the pair Pauli (words 0, 1) and TGT's words 2, 3, the
 *   second CTL's words 2, 3 (its words 0, 1 are unused).  A block with linear depth ld has n + 3 n ld calls; C = the circuit's
 *   total.  Shot mode continues from call C as qhea_noise continues from call m: u from words 0, 1 of call C; bit i uses word
 *   (2 + i) mod 4 of call C + (2 + i) / 4; a bit that is 0 flips iff its word is < floor(readout01[i] 2^32), a bit that is 1 iff
 *   it is < floor(readout10[i] 2^32).
 * Estimators: expectation mode (sampling.shots = 0, T = sampling.trajectories) and shot mode (S = sampling.shots) of
 *   qhea_noise; stderr_out = sample deviation / sqrt(count).  The asymmetric readout is folded into expectation mode as
 *     h(k) = offset + coeff sum_i (bit_i(k) ? -(1 - 2 readout10[i]) : 1 - 2 readout01[i]),  or with ham_diag
 *     diag'[k] = sum_j prod_i c_i(bit_i(j) | bit_i(k)) diag[j],  c_i = bit i's 2 x 2 confusion matrix, k the true string.
 * Summation, each order a function of n and the number of values per row only:
 *   1. tiles of 64 trajectories, a row's tile sums added in tile order; inside a tile, n = 2..6: slot j of the 64 / 2^n slots
 *      adds trajectories j, j + slots, .. in that order and the slots are added in slot order; n = 7..9: trajectory order;
 *   2. the masked sum M of a damping site (|psi_k|^2 over the k whose wire is |1>, zero elsewhere): n = 2..6 the xor butterfly
 *      over the trajectory's 2^n lanes, offsets 2^(n-1), .., 1; n = 7..9 per lane the terms k = l + 64 r in the order
 *      r = 0, 1, .., then the butterfly over the 64 lanes, offsets 32, .., 1 (wires 6..8 select registers, not lanes);
 *   3. read-out: value = (sum_k p_k h'(k)) / (sum_k p_k) + offset term, p_k = |psi_k|^2 of the unnormalised final state, both
 *      sums in the order of 2 (unmasked); h' is built by one launch: the sum over i in the order i = 0..n-1 times coeff, or
 *      diag' bit by bit, h <- (1 - e) h + e h[k ^ 2^i] for i = 0..n-1 with e = readout01[i] where bit i of k is 0 and
 *      readout10[i] where it is 1;
 *   4. shot mode: the first k with u sum_k p_k < cdf[k] (the total as in 3); cdf in index order for n = 2..6, and for n = 7..9
 *      the blocks-of-64 Hillis-Steele scan of qhea_model_forward_noisy_wide; if there is none, the last k with p_k > 0.
 * No floating-point atomics; results are bitwise reproducible and independent of the batch, the grid and the chunking.
 * Scope: n = 2..9, both models, trainable or fixed frequency, Z / X / Y and ham_diag read-outs.  Out of scope: n = 10..12
 * (QHEA_EUNSUPPORTED here: with the state in LDS the sites are laid out differently, and that range is
 * qhea_model_forward_noisy_device_wide below); gradients and training through trajectories; thermal population, crosstalk and
 * routing, as above.
 * Errors, all before anything is launched, outputs untouched: QHEA_EINVAL for the cases of
 * qhea_model_forward_noisy_device_exact (by the same code) and for a bad sampling record (NULL, shots < 0, trajectories < 1 in
 * expectation mode, more than 2^32 - 1 values per row); then QHEA_EUNSUPPORTED for n >= 10; then the errors of
 * qhea_model_forward_noisy (and QHEA_EINVAL for batch * ceil(values / 64) > 2^31 - 1).
 * Launches: the prep kernel, one kernel that writes the per-site constants (and expectation mode's h') into the workspace, the
 * trajectory kernel, the finishing kernel of qhea_model_forward_noisy; no allocation, no synchronisation (hipGraph-capturable).
 */
typedef struct qhea_sampling {
    int64_t  shots;             /* 0: expectation mode; S >= 1: shot mode (one trajectory per shot) */
    int64_t  trajectories;      /* expectation mode: T >= 1 (ignored in shot mode)                  */
    uint64_t seed;
} qhea_sampling;

int    qhea_device_noise_jump_tables(int n, const qhea_device_noise* dn /*HOST*/, double* jump /*HOST [4][n][2] = (gamma, pz)*/);
/* DEVICE scratch bytes for qhea_model_forward_noisy_device on `batch` rows (0 on a bad descriptor or sampling record, or n >= 10). */
size_t qhea_model_noisy_device_workspace_bytes(const qhea_model_desc* desc, int64_t batch, const qhea_sampling* sampling);
int    qhea_model_forward_noisy_device(const qhea_model_desc* desc, int64_t row0, int64_t batch,
                                       const double* branch /*DEVICE [B,branch_in]*/, const double* trunk /*DEVICE [B,trunk_in] or NULL*/,
                                       const double* params /*DEVICE flat*/, const double* ham_diag /*DEVICE [2^n] or NULL*/,
                                       const qhea_device_noise* dn /*HOST*/, const qhea_sampling* sampling /*HOST*/,
                                       double* pred /*DEVICE [B]*/, double* stderr_out /*DEVICE [B] or NULL*/,
                                       void* workspace, size_t workspace_bytes, void* stream);

/*
 * qhea_model_forward_noisy_device for n = 10..12, where the state lives in LDS (one workgroup of 2^(n-4) threads per tile of 64
 * trajectories, the layout of qhea_model_forward_noisy_wide).  Model, unravelling, random stream (calls, words, counter, shot
 * mode's continuation from call C), estimators and stderr_out are those of qhea_model_forward_noisy_device, word for word; the
 * two calls answer for disjoint qubit counts.  What differs:
 * Scope: n = 10..12; n <= 9 returns QHEA_EUNSUPPORTED (qhea_model_noisy_device_wide_workspace_bytes: 0).
 * Errors: those of qhea_model_forward_noisy_device in its order, with "n <= 9" in the place of "n >= 10".
 * Summation, each order a function of n and the number of values per row only:
 *   1. tiles of 64 trajectories in trajectory order, a row's tile sums added in tile order (the finishing kernel);
 *   2. the masked sum M of a damping site.  Thread t of the 2^(n-4) holds, in the pass where the site sits, the 16 amplitudes
 *      k = (t >> A) << (A + 4) | (t & (2^A - 1)) | J << A, J = 0..15, of the state as it is stored (a sub-layer's state keeps
 *      the labels it had before the CNOT ring until the ring's last slot; sampled Paulis and fired jumps are carried as a
 *      frame): A = 4 floor(q / 4) for site ENC_q / ROT_q, except in the last pass of n = 10 and n = 11, which holds bits
 *      n - 4 .. n - 1 (A = 6: q = 8, 9; A = 7: q = 8, 9, 10); A = n - 4 for the 2 n sites of the ring.  The masked terms are
 *      added in the order J = 0..15 (zero where the wire reads |0>), then over the 64 lanes of a wave by the xor butterfly,
 *      offsets 32, .., 1, then the n = 11: 2, n = 12: 4 waves in wave order.  Every site has its own sum: the TGT / CTL pair
 *      of a slot shares none;
 *   3. read-out: value = (sum_k p_k h'(k)) / (sum_k p_k) + offset term; thread t adds the 16 basis states 16 t .. 16 t + 15 in
 *      index order, then the butterfly and the waves as in 2, both sums; h' is built as for n = 2..9;
 *   4. shot mode: the first k with u S < cdf[k], S = sum_k p_k as in 3, else the last k with p_k > 0; cdf[k]: chunks of 16
 *      summed in index order, a Hillis-Steele scan of the chunk sums over each wave (distances 1, 2, .., 32), wave totals added
 *      in wave order -- the cdf of qhea_model_forward_noisy_wide for n = 10..12.
 * No floating-point atomics; results are bitwise reproducible and independent of the batch, the grid and the chunking.
 * Launches: the prep kernel, one kernel that writes this call's table of per-site constants (and expectation mode's h') into the
 * workspace, the trajectory kernel, the finishing kernel of qhea_model_forward_noisy; a linear chain, no allocation, no
 * synchronisation (hipGraph-capturable).
 */
/* DEVICE scratch bytes for qhea_model_forward_noisy_device_wide on `batch` rows (0 on a bad descriptor or sampling record, or n <= 9). */
size_t qhea_model_noisy_device_wide_workspace_bytes(const qhea_model_desc* desc, int64_t batch, const qhea_sampling* sampling);
int    qhea_model_forward_noisy_device_wide(const qhea_model_desc* desc, int64_t row0, int64_t batch,
                                            const double* branch /*DEVICE [B,branch_in]*/, const double* trunk /*DEVICE [B,trunk_in] or NULL*/,
                                            const double* params /*DEVICE flat*/, const double* ham_diag /*DEVICE [2^n] or NULL*/,
                                            const qhea_device_noise* dn /*HOST*/, const qhea_sampling* sampling /*HOST*/,
                                            double* pred /*DEVICE [B]*/, double* stderr_out /*DEVICE [B] or NULL*/,
                                            void* workspace, size_t workspace_bytes, void* stream);

/*
 * Training under the calibrated device noise model at n = 7..9, where qhea_model_loss_grad_noisy_device_exact's density matrix
 * no longer fits: the MSE loss of the quantum-jump estimate (qhea_model_forward_noisy_device, expectation mode) and an unbiased
 * gradient of it.
 *
 * The estimator.  Fix a row and a random stream.  Trajectory k applies, in circuit order, the gates, the sampled Paulis, the
 * dephasing flips and at every damping site one of two fixed linear operators, the unnormalised ones of the forward call:
 * K0 = diag(1, sqrt(1 - gamma)) (no jump) or L = |0><1| (jump).  With psi~_k the unnormalised final state, N2_k = <psi~_k|psi~_k>
 * and num_k = <psi~_k|h'|psi~_k> (h' the read-out weights with the asymmetric readout folded in), the probability of pattern k is
 * c_k N2_k with c_k free of the parameters, the trajectory's value is num_k / N2_k, and the exact value is sum_k c_k num_k.  Hence
 * d pred / d theta = sum_k c_k d num_k = E_k[ d num_k / N2_k ]:
 *   the gradient of the unnormalised numerator is taken with the fired pattern held fixed and divided by the final N2.  The
 *   norm is not differentiated, and the jump decisions are not differentiated.  (The score-function term of the pattern's
 *   probability and the derivative of 1 / N2 cancel exactly; differentiating the normalised value with the pattern fixed is
 *   biased.)
 *   pred_b       = what qhea_model_forward_noisy_device returns for global row row0 + b under the same dn and sampling (to
 *                  rounding, not bitwise: the tiles below are this call's own): the mean of the T trajectory values + bias;
 *   loss         = sum_b (pred_b - y_b)^2 * inv_batch_total;
 *   grad[0..P)   = sum_b 2 (pred_b - y_b) inv_batch_total * (the unbiased d pred_b / d params above), in the flat layout of
 *                  qhea_model_loss_grad;  grad[P] = sum_b (pred_b - y_b)^2;  grad[P+1] = sum_b y_b^2.
 *   As in qhea_model_loss_grad_noisy_wide the expectation of the sampled loss is the exact MSE + inv_batch_total sum_b Var_b / T,
 *   and pred_b and d pred_b are taken from the same trajectories: the loss gradient is the exact one plus sampling noise plus a
 *   term of order 1 / T.  The estimator is stated here, not corrected.
 * The walk.  Per trajectory the forward walk of qhea_model_forward_noisy_device (n = 7..9), word for word; then
 * lambda = h' psi~ / N2 behind the read-out's basis change; then lambda goes back through the ADJOINTS of the fixed operators
 * (K0^dagger = K0, L^dagger = |1><0|, each with the polarity of the Pauli frame at its site; a segment's frame X^x Z^z is its own
 * inverse up to the sign (-1)^parity(x & z), which is applied) and psi goes back beside it -- by the gates' inverses and K0^-1, and at a fired
 * site, where L has no inverse, from a snapshot: the forward walk keeps psi~ at the start of every block, and the state before
 * the jump is that snapshot walked forward again to the site (at most one block per fired jump).  Per fused RY RZ RY the sums
 * Im<lambda|sigma|psi>, sigma = X, Y, Z, behind the gate; per encoding RX the X sum behind it.  The exact power-of-two rescale
 * of the forward walk is crossed by both (psi 2^-100, lambda 2^100), so psi is always in the scale the forward walk had there
 * and every product is unchanged; lambda stays finite while fewer than 9 rescales lie behind a point of the circuit (N2 of a
 * pattern below 2^-1800, which no supported shape reaches).
 * Random numbers: exactly those of the forward call (Philox calls, words, thresholds, the rule u N2 < gamma M) and only in the
 * forward walk.  It records per segment (a block's encoding sites, or a sub-layer) four 32-bit words: which of its <= 27
 * damping sites fired (and whether the rescale behind it did), the frame's polarity at each site, and the segment's final
 * frame (X mask, Z mask).  The reverse walk and the re-walks read these words: no jump is decided twice.
 * Summation, each order a function of n, the shape and T only:
 *   1. a trajectory's value, the masked sums and N2: as in qhea_model_forward_noisy_device (2., 3., n = 7..9); its inner products
 *      as in qhea_model_loss_grad_noisy_wide (1.);
 *   2. a row's trajectories go in tiles of 4; inside a tile values and inner products are added in trajectory order;
 *   3., 4. the tiles, the angles' derivatives and the rows as in qhea_model_loss_grad_noisy_wide (3., 4.).
 * Workspace: a function of the shape, the batch and T only, never of how many jumps fire: the tables, (E + 3 n blk) doubles per
 * (row, tile) and per row, and per launched wave -- min(batch * ceil(T / 4), 2048) of them, which take the (row, tile) items in
 * a grid-stride loop -- one state per block and 1 KiB per segment.  An item's result does not depend on the wave that walks it.
 * No trajectory is dropped, truncated or capped.
 * qhea_model_train_steps_noisy_device: the arguments of qhea_model_train_steps_noisy_wide with dn and sampling in the place of
 * noise.  Step i has the Adam count t = first_step + i, draws from the stream keyed sampling->seed + t (mod 2^64) with global rows
 * row_begin[i] + r, and is bitwise qhea_model_loss_grad_noisy_device with that seed and row0 = row_begin[i] followed by
 * qhea_adam_step; a run resumed at first_step reproduces an uninterrupted one.  The workspace must fit the largest step.
 * Scope: n = 7..9, one device, sampling.shots = 0, both models, trainable or fixed frequency, Z / X / Y and ham_diag read-outs.
 * Errors, all before anything is launched and with the outputs untouched, in the order of qhea_model_forward_noisy_device: a bad
 * descriptor; QHEA_EINVAL for a bad device setting, a NULL sampling, shots != 0 (shot mode has no such gradient) and
 * trajectories < 1; QHEA_EUNSUPPORTED for n <= 6 (qhea_model_loss_grad_noisy_device_exact) and n >= 10; QHEA_EINVAL for a bad
 * read-out, a negative batch or row0, first_step < 1, NULL arrays; QHEA_EINVAL for a site with 1 - gamma == 0 in fp64, which no
 * inverse undoes (qhea_device_noise_singular_site names it: 1 and *site (0 ENC, 1 ROT, 2 CTL, 3 TGT), *wire for the first such
 * site, 0 if there is none); QHEA_EINVAL for batch * ceil(T / 4) > 2^31 - 1; QHEA_EWORKSPACE.  An empty batch (or n_steps = 0)
 * returns QHEA_OK.  There is no amplification guard: K0^-1 scales one half of the state by 1 / sqrt(1 - gamma), and with it the
 * rounding already there; the relative error of a trajectory's gradient grows with the product of those factors over a wire's
 * unfired sites since the last fired one (DESIGN.md 7p has the table; quanonet_amd.noise.JUMP_GAMMA_MAX is the Python layer's bound).
 * Launches: per CALL the kernel that writes the per-site constants and h'; per step the prep kernel, the trajectory kernel, the
 * fold kernel and the reduce kernel (with Adam in train_steps) of qhea_model_loss_grad_noisy_wide.  A linear chain, no
 * allocation, no synchronisation (hipGraph-capturable).  No atomics and fixed orders: results are bitwise reproducible.
 */
int    qhea_device_noise_singular_site(int n, const qhea_device_noise* dn /*HOST*/, int* site /*HOST or NULL*/, int* wire /*HOST or NULL*/);
/* DEVICE scratch bytes for the two calls on (at most) `batch` rows (0 on a bad descriptor or sampling record, shots != 0, or n
 * outside 7..9). */
size_t qhea_model_noisy_device_grad_workspace_bytes(const qhea_model_desc* desc, int64_t batch, const qhea_sampling* sampling);
int    qhea_model_loss_grad_noisy_device(const qhea_model_desc* desc, int64_t row0, int64_t batch,
                                         const double* branch, const double* trunk, const double* y /*DEVICE [B]*/,
                                         const double* params, const double* ham_diag,
                                         const qhea_device_noise* dn /*HOST*/, const qhea_sampling* sampling /*HOST: shots = 0*/,
                                         double inv_batch_total, double* grad /*DEVICE [P+2]*/, double* pred /*DEVICE [B] or NULL*/,
                                         void* workspace, size_t workspace_bytes, void* stream);
int    qhea_model_train_steps_noisy_device(const qhea_model_desc* desc, int64_t n_steps, const int64_t* row_begin /*HOST [n_steps+1]*/,
                                           const double* branch /*DEVICE*/, const double* trunk /*DEVICE or NULL*/,
                                           const double* y /*DEVICE*/, double* params /*DEVICE flat, updated in place*/,
                                           const double* ham_diag, const qhea_device_noise* dn /*HOST*/,
                                           const qhea_sampling* sampling /*HOST*/,
                                           const double* inv_batch_total /*HOST [n_steps]*/,
                                           double* grad /*DEVICE [n_steps][grad_stride]*/, int64_t grad_stride,
                                           double* exp_avg, double* exp_avg_sq, int64_t first_step, double lr, double beta1,
                                           double beta2, double eps, double weight_decay, void* workspace,
                                           size_t workspace_bytes, void* stream);

/*
 * qhea_model_loss_grad_noisy_device_lds / qhea_model_train_steps_noisy_device_lds (library version 610): the two calls above for
 * n = 10, 11 and 12, where psi and lambda live in LDS (hea_noise_device_grad_lds.hip).  The arguments, the quantity, the
 * estimator (d pred_b = E_k[d num_k / N2_k] with the fired pattern held fixed; neither the norm nor the jump decisions are
 * differentiated), the loss's Var / T term (stated, not corrected), the errors and their order, train_steps' stream keys
 * (sampling->seed + first_step + i, mod 2^64, global rows row_begin[i] + r; bitwise the single call followed by qhea_adam_step)
 * and the launch chain are those of qhea_model_loss_grad_noisy_device; qhea_model_loss_grad_noisy_device itself keeps returning
 * QHEA_EUNSUPPORTED at n >= 10, and these return it at n <= 9.
 *   pred_b = what qhea_model_forward_noisy_device_wide returns for global row row0 + b under the same dn and sampling, to
 *   rounding (the tiles below are this call's own).
 * Random numbers: exactly those of qhea_model_forward_noisy_device_wide (Philox calls, words, thresholds, u N2 < gamma M), drawn
 * only in the forward walk, which is that call's code.  Per segment it records eight 32-bit words in the workspace: which of
 * the segment's <= 36 sites fired (site q < n the segment's own site of wire q, n + 2 j the TGT and n + 2 j + 1 the CTL site of
 * slot j: bits 0..31 in word 0, 32..35 in word 1, whose bit 31 says that the rescale behind the segment fired), the frame's X
 * bit on the site's wire when the site was reached (words 2, 3), and the frame the segment's last store applied (word 4 the X
 * mask in LDS slot bits, word 5 the Z mask pulled back through the ring); words 6, 7 are unused.  The reverse walk and the
 * re-walks read them: nothing is decided or drawn twice.
 * The walk is that of qhea_model_loss_grad_noisy_device in the LDS layout: 2^(n-4) threads, 16 amplitudes per thread and pass at
 * every n and in both directions; a site is a diagonal step on those 16 with the forward's stored-bit masks and the recorded
 * polarity (no jump: psi by 1 / sqrt(1 - gamma), lambda by sqrt(1 - gamma); jump: lambda by the projector, its X sits in the
 * recorded frame, psi from the block's snapshot walked forward to the site).  A segment's last store and the reverse walk's
 * first gather are exact inverses (both drop the frame's sign (-1)^parity(x & z), and so does every re-walk), so no sign is
 * applied here.
 * Summation, each order a function of n, the shape and T only:
 *   1. a site's masked sum and a trajectory's num and N2: as in qhea_model_forward_noisy_device_wide (the thread's 16 terms in
 *      local-index order, the wave by the butterfly with offsets 32 .. 1, the waves in wave order);
 *   2. an inner product: the thread's pairs in local-index order as FMA chains, the wave by the transposing butterfly over lane
 *      bits 0 .. 5, the waves in wave order (as qhea_model_loss_grad_noisy_lds, 1., with 16 amplitudes per thread at every n);
 *   3. a row's trajectories go in tiles of 2; inside a tile values and inner products are added in trajectory order;
 *   4., 5. the tiles, the angles' derivatives and the rows as in qhea_model_loss_grad_noisy_wide (3., 4.).
 * Workspace: a function of the shape, the batch and T only, never of how many jumps fire: the tables, (E + 3 n blk) doubles per
 * (row, tile) and per row, and per launched workgroup -- min(batch * ceil(T / 2), qhea_noisy_device_lds_grad_max_workgroups(n))
 * of them, which take the (row, tile) items in a grid-stride loop -- 2^n * 16 bytes per block and 32 bytes per segment.  An
 * item's result does not depend on the workgroup that walks it, so results do not depend on batch, grid or chunking.  No
 * trajectory is dropped, truncated or capped.
 * qhea_noisy_device_lds_grad_max_workgroups: the launch cap (1024 / 512 / 256 at n = 10 / 11 / 12: what 256 compute units keep
 * resident), 0 outside 10..12.
 */
/* DEVICE scratch bytes for the two calls on (at most) `batch` rows (0 on a bad descriptor or sampling record, shots != 0, or n
 * outside 10..12). */
size_t qhea_model_noisy_device_lds_grad_workspace_bytes(const qhea_model_desc* desc, int64_t batch, const qhea_sampling* sampling);
int    qhea_noisy_device_lds_grad_max_workgroups(int n);
int    qhea_model_loss_grad_noisy_device_lds(const qhea_model_desc* desc, int64_t row0, int64_t batch,
                                             const double* branch, const double* trunk, const double* y /*DEVICE [B]*/,
                                             const double* params, const double* ham_diag,
                                             const qhea_device_noise* dn /*HOST*/, const qhea_sampling* sampling /*HOST: shots = 0*/,
                                             double inv_batch_total, double* grad /*DEVICE [P+2]*/, double* pred /*DEVICE [B] or NULL*/,
                                             void* workspace, size_t workspace_bytes, void* stream);
int    qhea_model_train_steps_noisy_device_lds(const qhea_model_desc* desc, int64_t n_steps, const int64_t* row_begin /*HOST [n_steps+1]*/,
                                               const double* branch /*DEVICE*/, const double* trunk /*DEVICE or NULL*/,
                                               const double* y /*DEVICE*/, double* params /*DEVICE flat, updated in place*/,
                                               const double* ham_diag, const qhea_device_noise* dn /*HOST*/,
                                               const qhea_sampling* sampling /*HOST*/,
                                               const double* inv_batch_total /*HOST [n_steps]*/,
                                               double* grad /*DEVICE [n_steps][grad_stride]*/, int64_t grad_stride,
                                               double* exp_avg, double* exp_avg_sq, int64_t first_step, double lr, double beta1,
                                               double beta2, double eps, double weight_decay, void* workspace,
                                               size_t workspace_bytes, void* stream);

/*
 * qhea_model_forward over `n_chunks` consecutive row ranges [row_begin[i], row_begin[i+1]) of the same arrays with the
 * SAME parameters -- the chunk loop of PTSolver.evaluate / infer.predict (solvers/solver_pt.py:299-310, infer.py:274-289) in
 * one host call.  The layer records depend on the parameters alone, so one preparation launch serves all chunks of
 * equal size; results are bitwise those of the single calls.  The workspace must fit the largest chunk.
 */
int qhea_model_forward_chunks(const qhea_model_desc* desc, int64_t n_chunks, const int64_t* row_begin /*HOST [n_chunks+1]*/,
                              const double* branch /*DEVICE*/, const double* trunk /*DEVICE or NULL*/,
                              const double* params /*DEVICE flat*/, const double* ham_diag, double* pred /*DEVICE [rows]*/,
                              void* workspace, size_t workspace_bytes, void* stream);

/*
 * One fused loss + gradient evaluation:
 *   pred_b = model(...);  loss contribution = (pred_b - y_b)^2 * inv_batch_total;
 *   grad[0..P) = d/dparams sum_b (pred_b - y_b)^2 * inv_batch_total;  grad[P] = sum_b (pred_b-y_b)^2;
 *   grad[P+1] = sum_b y_b^2.
 * inv_batch_total = 1 / (GLOBAL batch size): a rank's shard passes the global size, and a SUM over
 * ranks reproduces MSELoss(mean) gradients of the whole batch (solvers/solver_pt.py:232-236).
 * pred may be NULL.
 */
int qhea_model_loss_grad(const qhea_model_desc* desc, int64_t batch,
                         const double* branch, const double* trunk, const double* y /*DEVICE [B]*/,
                         const double* params, const double* ham_diag, double inv_batch_total,
                         double* grad /*DEVICE [P+2]*/, double* pred /*DEVICE [B] or NULL*/,
                         void* workspace, size_t workspace_bytes, void* stream);

/*
 * Single-device training step: qhea_model_loss_grad followed by qhea_adam_step on the same flat vectors, with the
 * Adam update applied by the very thread of the reduce kernel that finishes each gradient -- three launches
 * (prep, circuit, reduce+Adam) for `pred = model(...); loss = MSE(pred, y); loss.backward(); optimizer.step()`
 * (solvers/solver_pt.py:232-236).  Bitwise the same parameters as the two separate calls.  Data-parallel runs
 * keep the two calls, with the gradient all-reduce between them.  grad still receives [gradients | sse | sum y^2].
 */
int qhea_model_train_step(const qhea_model_desc* desc, int64_t batch,
                          const double* branch, const double* trunk, const double* y /*DEVICE [B]*/,
                          double* params /*DEVICE flat, updated in place*/, const double* ham_diag,
                          double inv_batch_total, double* grad /*DEVICE [P+2]*/, double* pred /*DEVICE [B] or NULL*/,
                          double* exp_avg /*DEVICE [P]*/, double* exp_avg_sq /*DEVICE [P]*/, int64_t step,
                          double lr, double beta1, double beta2, double eps, double weight_decay,
                          void* workspace, size_t workspace_bytes, void* stream);

/*
 * `n_steps` consecutive qhea_model_train_step calls over CONTIGUOUS rows, issued from one host call: the inner loop of
 * one epoch (solvers/solver_pt.py:226-241, after the epoch's rows have been gathered in batch order).  Step i takes
 * rows [row_begin[i], row_begin[i+1]) of branch / trunk / y, weights its residuals with inv_batch_total[i], leaves its
 * [P+2] buffer (gradients | sse | sum y^2) at grad + i * grad_stride and applies Adam update number first_step + i.
 * Nothing is synchronised; results are bitwise those of the single calls.  The workspace must fit the largest step.
 */
int qhea_model_train_steps(const qhea_model_desc* desc, int64_t n_steps, const int64_t* row_begin /*HOST [n_steps+1]*/,
                           const double* branch /*DEVICE*/, const double* trunk /*DEVICE or NULL*/,
                           const double* y /*DEVICE*/, double* params /*DEVICE flat*/, const double* ham_diag,
                           const double* inv_batch_total /*HOST [n_steps]*/, double* grad /*DEVICE [n_steps][grad_stride]*/,
                           int64_t grad_stride, double* exp_avg, double* exp_avg_sq, int64_t first_step, double lr,
                           double beta1, double beta2, double eps, double weight_decay, void* workspace,
                           size_t workspace_bytes, void* stream);

/*
 * One Adam update of the flat parameter vector, in place, in ONE launch.  Same arithmetic as
 * torch.optim.Adam (amsgrad=False, maximize=False; the reference's optimizer, solvers/solver_pt.py:149-163):
 *   m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
 * with g += weight_decay * p first when weight_decay != 0.  `step` is the 1-based update count t.
 */
int qhea_adam_step(int64_t n, double* params /*DEVICE*/, const double* grads /*DEVICE*/,
                   double* exp_avg /*DEVICE*/, double* exp_avg_sq /*DEVICE*/, int64_t step,
                   double lr, double beta1, double beta2, double eps, double weight_decay, void* stream);

/*
 * Data-parallel gradient exchange (the reference has no multi-device step -- this replaces the
 * `all_reduce` + `optimizer.step()` pair a DistributedDataParallel port of solvers/solver_pt.py:232-237 would run).
 * Every rank owns ONE exchange buffer of fine-grained device memory that every other rank maps through hipIpc; one
 * one-workgroup kernel per rank and step writes the rank's flat buffer [gradients | sse | sum y^2] into every other rank's
 * buffer -- each value as two 8-byte words that carry the exchange's sequence number, so that a value validates itself
 * and nothing has to be drained or flagged --, polls its own buffer for the other ranks' words, sums in rank order (bitwise
 * identical on every rank, reproducible) and applies Adam -- no collective-library launch and no separate optimizer launch
 * on the step's critical path.  Set-up (once): qhea_dp_alloc -> qhea_dp_export -> exchange the 64-byte handles by any means
 * (torch.distributed.all_gather_object) -> qhea_dp_import each peer's.  The library retains nothing: the caller
 * owns the buffer and the mapped pointers and passes them to every call.
 */
#define QHEA_DP_MAX_RANKS    16
#define QHEA_DP_HANDLE_BYTES 64
size_t qhea_dp_buffer_bytes(int64_t n_values, int world);
/* allocate (fine-grained, zeroed) / free this rank's exchange buffer for `n_values` doubles per rank */
int qhea_dp_alloc(int64_t n_values, int world, void** buffer /*out: DEVICE*/);
int qhea_dp_free(void* buffer);
/* inter-process handle of an exchange buffer (QHEA_DP_HANDLE_BYTES bytes, host), and a peer's buffer mapped from one */
int qhea_dp_export(void* buffer /*DEVICE*/, void* handle64 /*HOST out*/);
int qhea_dp_import(const void* handle64 /*HOST*/, void** peer_buffer /*out: DEVICE pointer valid in this process*/);
int qhea_dp_close(void* peer_buffer);
/*
 * out[i] = sum over ranks r = 0..world-1 (in that order) of rank r's local[i], i < n_values; then, if params != NULL,
 * the Adam update of qhea_adam_step on params[0..n_params) with gradient out[i].  `buffers` is a HOST array of `world`
 * device pointers: buffers[rank] this rank's own buffer, the others as returned by qhea_dp_import.  `seq` counts the
 * exchanges on these buffers from 1 and must be the same on every rank for the same step; `local` and `out` may be
 * the same array.  A rank that does not hear from every other rank within `timeout_ms` writes NaN to `out`, skips the
 * update and raises the error that qhea_dp_status reports.
 */
int qhea_dp_allreduce_adam(int rank, int world, void* const* buffers /*HOST array of DEVICE pointers*/,
                           int64_t n_values, int64_t seq, const double* local /*DEVICE*/, double* out /*DEVICE*/,
                           int64_t n_params, double* params /*DEVICE or NULL*/, double* exp_avg, double* exp_avg_sq,
                           int64_t step, double lr, double beta1, double beta2, double eps, double weight_decay,
                           double timeout_ms, void* stream);
/*
 * waits for `stream`; QHEA_EEXCHANGE if an exchange on this buffer failed since the last call.  A timeout is fatal on
 * EVERY rank: the rank whose wait overran raises a sticky word in every rank's buffer, and from then on every exchange on
 * these buffers -- the late rank's included -- fails (NaN results, no update) and this call keeps returning
 * QHEA_EEXCHANGE; the replicas cannot drift apart silently.  Free and re-create the buffers to start over.
 */
int qhea_dp_status(void* buffer /*DEVICE: this rank's own*/, void* stream);

/*
 * The data-parallel training step with the exchange INSIDE the reduce kernel: qhea_model_train_steps for `world` ranks.
 * Step i of this rank trains on its shard rows [row_begin[i], row_begin[i+1]) (never empty) with residual weight
 * inv_batch_total[i] = 1 / GLOBAL batch; every block of the step's reduce kernel publishes the gradients it has just
 * summed to the peers' exchange buffers (exchange number first_seq + i; the qhea_dp_* buffers above, allocated for
 * dp_values >= P + 2 doubles), waits for the peers' blocks, adds the contributions in rank order, leaves the GLOBAL
 * [gradients | sse | sum y^2] in grad + i*grad_stride, applies Adam and -- between steps of equal shard size on the
 * block-unrolled shapes -- writes the next step's layer records: two launches per step (circuit, reduce) instead of
 * prep + circuit + reduce + exchange.  Bitwise the results of qhea_model_loss_grad + qhea_dp_allreduce_adam.  Replaces the
 * `loss.backward(); all_reduce; optimizer.step()` a DistributedDataParallel port of solvers/solver_pt.py:232-237 would run.
 * Returns QHEA_EUNSUPPORTED -- before anything is launched -- when a shard is empty or the reduce grid would not be
 * resident at once (more blocks than CUs: its blocks wait for their peers' blocks): use qhea_model_loss_grad +
 * qhea_dp_allreduce_adam for such a run.  Failure semantics as qhea_dp_allreduce_adam / qhea_dp_status.
 */
int qhea_model_dp_train_steps(const qhea_model_desc* desc, int64_t n_steps, const int64_t* row_begin /*HOST [n_steps+1]*/,
                              const double* branch, const double* trunk, const double* y, double* params,
                              const double* ham_diag, const double* inv_batch_total /*HOST [n_steps]*/,
                              double* grad /*DEVICE [n_steps, grad_stride]*/, int64_t grad_stride,
                              double* exp_avg, double* exp_avg_sq, int64_t first_step, double lr, double beta1,
                              double beta2, double eps, double weight_decay,
                              int rank, int world, void* const* buffers /*HOST array of DEVICE pointers*/,
                              int64_t dp_values, int64_t first_seq, double timeout_ms,
                              void* workspace, size_t workspace_bytes, void* stream);

/*
 * Model ensemble: R = n_models independent models of ONE descriptor trained side by side, each step of all R members as one
 * launch per kernel (member = the grid's second dimension) -- a seed sweep of one configuration on one device.  Replaces
 * the reference's concurrent seed processes (one training process per seed, each issuing its own small launches).
 * Member m has its own rows (branch / trunk / y: member m's start at m * row_begin[n_steps] rows), parameters, Adam
 * moments (params / exp_avg / exp_avg_sq: [n_models][P]) and gradient rows (grad + (m * n_steps + i) * grad_stride for
 * step i); all members share the schedule row_begin / inv_batch_total, the step count and the hyper-parameters.
 * Results are bitwise those of n_models qhea_model_train_steps calls, one per member, made under the backward variant the
 * ensemble chose: the kernels are chosen as for ONE batch of n_models x B rows (qhea_set_backward_variant applies).
 * n >= 10 (n_models > 1): one launch per kernel too, the member form of the workgroup-resident backward kernel (one
 * workgroup per sample and member).  Other shapes the n <= 5 ZYZ kernels do not take (n = 6..9, first-generation variants,
 * shapes not eligible) run as n_models consecutive qhea_model_train_steps calls on the same stream, one workspace slice
 * each.  An overrun in any member is
 * reported by qhea_check_status on this workspace.  Workspace: qhea_model_ensemble_workspace_bytes for every batch size
 * of the schedule (the largest of those).  Bytes 64..111 of every member's slice hold that member's hyper-parameters for the
 * one-launch path (written by the call itself; qhea_model_sweep_train_steps below).
 */
size_t qhea_model_ensemble_workspace_bytes(const qhea_model_desc* desc, int64_t n_models, int64_t batch);
int qhea_model_ensemble_train_steps(const qhea_model_desc* desc, int64_t n_models, int64_t n_steps,
                                    const int64_t* row_begin /*HOST [n_steps+1], the same schedule for every member*/,
                                    const double* branch, const double* trunk, const double* y /*DEVICE, [n_models][rows]*/,
                                    double* params /*DEVICE [n_models][P]*/, const double* ham_diag /*shared*/,
                                    const double* inv_batch_total /*HOST [n_steps]*/,
                                    double* grad /*DEVICE [n_models][n_steps][grad_stride]*/, int64_t grad_stride,
                                    double* exp_avg /*DEVICE [n_models][P]*/, double* exp_avg_sq, int64_t first_step,
                                    double lr, double beta1, double beta2, double eps, double weight_decay,
                                    void* workspace, size_t workspace_bytes, void* stream);

/*
 * Model sweep: qhea_model_ensemble_train_steps for members that also differ in their read-out, fixed encoding scale and Adam
 * learning rate -- an ablation grid of one circuit shape (the reference's reproduce_hamiltonian.sh / reproduce_benchmarks1.sh
 * cells: --ham_pauli, --ham_bound, --ham_diag, --scale_coeff, --learning_rate x seeds) trained as one launch per kernel.
 * `desc` fixes the shape only (model, n_qubits, net, input widths, trainable_freq); its ham_pauli, scale_coeff, ham_offset
 * and ham_coeff are NOT used: member m reads out members[m].ham_pauli with H = ham_offset + ham_coeff * sum P_i, or
 * diag(ham_diag + m * 2^n) when ham_diag != NULL (then every member must read out Z), encodes with members[m].scale_coeff
 * when trainable_freq == 0, and takes Adam steps of members[m].lr (finite, >= 0; beta1, beta2, eps, weight_decay are shared).
 * The other arguments are qhea_model_ensemble_train_steps' (same layouts, same workspace rules).  `members` is read before
 * the call returns; the table reaches the device as kernel arguments (one small launch per 64 members and call), so the call
 * stays hipGraph-capturable.  Results: member m's are bitwise those of qhea_model_train_steps with m's descriptor (desc with
 * m's scale, offset, coeff, Pauli), lr = members[m].lr and ham_diag + m * 2^n, under the backward variant the sweep chose:
 * the kernels are chosen as for ONE batch of n_models x B rows, and as for an X / Y model if any member reads out X or Y.
 * n >= 10 takes the one-launch path of the workgroup-resident kernels as in qhea_model_ensemble_train_steps; other shapes
 * outside the one-launch path run as n_models consecutive qhea_model_train_steps calls with the members' descriptors.
 */
typedef struct qhea_member_hparams {
    double  scale_coeff;            /* the member's fixed encoding scale (trainable_freq == 0); ignored otherwise */
    double  ham_offset, ham_coeff;  /* H = offset + coeff * sum P_i                                               */
    double  lr;                     /* this call's Adam learning rate for the member                              */
    int32_t ham_pauli;              /* QHEA_PAULI_*                                                               */
    int32_t reserved;               /* 0                                                                          */
} qhea_member_hparams;

size_t qhea_model_sweep_workspace_bytes(const qhea_model_desc* desc, int64_t n_models, int64_t batch);
int qhea_model_sweep_train_steps(const qhea_model_desc* desc, int64_t n_models,
                                 const qhea_member_hparams* members /*HOST [n_models]*/,
                                 const double* ham_diag /*DEVICE [n_models][2^n] or NULL*/,
                                 int64_t n_steps, const int64_t* row_begin /*HOST [n_steps+1], the same for every member*/,
                                 const double* branch, const double* trunk, const double* y /*DEVICE, [n_models][rows]*/,
                                 double* params /*DEVICE [n_models][P]*/, const double* inv_batch_total /*HOST [n_steps]*/,
                                 double* grad /*DEVICE [n_models][n_steps][grad_stride]*/, int64_t grad_stride,
                                 double* exp_avg /*DEVICE [n_models][P]*/, double* exp_avg_sq, int64_t first_step,
                                 double beta1, double beta2, double eps, double weight_decay,
                                 void* workspace, size_t workspace_bytes, void* stream);

/*
 * Depth sweep: qhea_model_sweep_train_steps for members whose circuits also differ in depth -- a capacity grid (the
 * reference's reproduce_capacity.sh / reproduce_circuit.sh / reproduce_scaling.sh: net_size = hb 2 ht 2 over hb x ht x seeds)
 * trained as one launch per kernel and step.  descs[m] is member m's descriptor.  The descriptors may differ only in their
 * depths: QuanONet net[0] (branch blocks) and net[2] (trunk blocks), HEAQNN net[0]; model, n_qubits, the other net entries,
 * the input widths and trainable_freq must be equal (else QHEA_EINVAL).  Their ham_pauli, scale_coeff, ham_offset and ham_coeff
 * are NOT used: read-out, fixed scale and lr are members[m]'s, as in qhea_model_sweep_train_steps.
 * Layouts: Pmax = the largest qhea_model_param_count of the members.  params, exp_avg, exp_avg_sq are [n_models][Pmax]: member
 * m's flat vector (the layout of its own descriptor) is at m * Pmax, the rest of its row is never read or written.  grad is
 * [n_models][n_steps][grad_stride], grad_stride >= Pmax + 2; member m's row holds its P_m gradients, then sse, sum y^2.
 * branch / trunk / y / ham_diag / row_begin / inv_batch_total as in qhea_model_sweep_train_steps.
 * n <= 9: every step is one launch per kernel (member = the grid's second dimension) of the first-generation kernels with the
 * packed backward, at any batch; member m's results are bitwise those of qhea_model_train_steps with m's sweep descriptor
 * (descs[m] with members[m]'s read-out and scale), lr = members[m].lr and ham_diag + m * 2^n under QHEA_BWD_PACKED.
 * n >= 10: the same, with the member form of the workgroup-resident backward kernel (one workgroup per sample and member).
 * Workspace:
 * qhea_model_depth_sweep_workspace_bytes for every batch size of the schedule (the largest of those); an overrun of any member
 * is reported by qhea_check_status on it.
 */
size_t qhea_model_depth_sweep_workspace_bytes(const qhea_model_desc* descs /*HOST [n_models]*/, int64_t n_models, int64_t batch);
int qhea_model_depth_sweep_train_steps(const qhea_model_desc* descs /*HOST [n_models]*/, int64_t n_models,
                                       const qhea_member_hparams* members /*HOST [n_models]*/,
                                       const double* ham_diag /*DEVICE [n_models][2^n] or NULL*/,
                                       int64_t n_steps, const int64_t* row_begin /*HOST [n_steps+1], the same for every member*/,
                                       const double* branch, const double* trunk, const double* y /*DEVICE, [n_models][rows]*/,
                                       double* params /*DEVICE [n_models][Pmax]*/, const double* inv_batch_total /*HOST [n_steps]*/,
                                       double* grad /*DEVICE [n_models][n_steps][grad_stride]*/, int64_t grad_stride,
                                       double* exp_avg /*DEVICE [n_models][Pmax]*/, double* exp_avg_sq, int64_t first_step,
                                       double beta1, double beta2, double eps, double weight_decay,
                                       void* workspace, size_t workspace_bytes, void* stream);

/*
 * Qubit sweep: qhea_model_depth_sweep_train_steps for members whose circuits also differ in qubit count -- a scaling grid (the
 * reference's reproduce_scaling.sh: Q2..Q8, each with its own hb x ht list, x seeds) trained side by side.  The descriptors may
 * differ in n_qubits (2..12) and in their depths; model, the input widths, trainable_freq and the linear depths (QuanONet
 * net[1] / net[3], HEAQNN net[1], net[2]) must be equal (else QHEA_EINVAL).  ham_diag is [n_models][2^nmax] (nmax = the largest
 * n_qubits): member m reads the first 2^n_m entries of its row.  params / exp_avg / exp_avg_sq / grad / read-out / scale / lr
 * and the per-member result as in qhea_model_depth_sweep_train_steps: member m's results are bitwise those of
 * qhea_model_train_steps with m's sweep descriptor under QHEA_BWD_PACKED; row tails beyond P_m are never read or written.
 * Members with n <= 9 share every step's launches: one prep launch, one backward launch per register class present (n = 2;
 * n = 3..6) whose workgroups take (member, sample group) from a work list and one per n = 7, 8, 9 present, one reduce launch
 * over every member's own roles.
 * Members with n >= 10 share them too: one backward launch per n = 10, 11, 12 present (the workgroup-resident kernel, one
 * workgroup per sample and member, longest chain first); their roles are in the one reduce launch.  Workspace:
 * qhea_model_qubit_sweep_workspace_bytes for the largest batch of the schedule; an overrun of any member is reported by
 * qhea_check_status on it.
 */
size_t qhea_model_qubit_sweep_workspace_bytes(const qhea_model_desc* descs /*HOST [n_models]*/, int64_t n_models, int64_t batch);
int qhea_model_qubit_sweep_train_steps(const qhea_model_desc* descs /*HOST [n_models]*/, int64_t n_models,
                                       const qhea_member_hparams* members /*HOST [n_models]*/,
                                       const double* ham_diag /*DEVICE [n_models][2^nmax] or NULL*/,
                                       int64_t n_steps, const int64_t* row_begin /*HOST [n_steps+1], the same for every member*/,
                                       const double* branch, const double* trunk, const double* y /*DEVICE, [n_models][rows]*/,
                                       double* params /*DEVICE [n_models][Pmax]*/, const double* inv_batch_total /*HOST [n_steps]*/,
                                       double* grad /*DEVICE [n_models][n_steps][grad_stride]*/, int64_t grad_stride,
                                       double* exp_avg /*DEVICE [n_models][Pmax]*/, double* exp_avg_sq, int64_t first_step,
                                       double beta1, double beta2, double eps, double weight_decay,
                                       void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QUANONET_HEA_H */
