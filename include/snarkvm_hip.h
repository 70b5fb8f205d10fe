/* snarkvm_hip.h - C ABI of the MI355X (gfx950) MSM / NTT backend for snarkVM.
 *
 * Part 1 is the drop-in boundary: the three symbols that `snarkvm-algorithms-cuda` binds
 * (reference: algorithms/cuda/src/lib.rs:42-69, defined by algorithms/cuda/cuda/snarkvm_api.cu:52-84).
 * A build of the reference with its `cuda` feature can link this library instead of the nvcc object
 * without touching any Rust caller (INTEGRATION.md shows the binding).
 *
 * Part 2 is an extension ABI (not in the reference): device-resident operands, SRS registration,
 * timing hooks.  Part 3 are test hooks.
 *
 * All functions are thread-safe and never unwind.  Concurrent callers (rayon workers: one commitment each) are handed
 * different (device, stream) lanes - the reference's resource channel, snarkvm.cu:84,146-150 - and block only when every
 * lane of every selected device is busy.  No torch / C++ types cross this boundary.
 */
#ifndef SNARKVM_HIP_H
#define SNARKVM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* sppark `cuda::Error` as seen by Rust (algorithms/cuda/src/lib.rs:20 `sppark::cuda_error!()`):
 * code == 0 means success; `message` is NULL or a malloc()ed C string that the caller frees
 * (build.rs:79 -DTAKE_RESPONSIBILITY_FOR_ERROR_MESSAGE).  Any non-zero code makes the Rust caller
 * fall back to its CPU path (msm/variable_base/mod.rs:39-43, fft/domain.rs:385-391). */
typedef struct {
    int32_t code;
    char *message;
} RustError;

enum NTTInputOutputOrder { NN = 0, NR = 1, RN = 2, RR = 3 }; /* lib.rs:22-28 */
enum NTTDirection { Forward = 0, Inverse = 1 };              /* lib.rs:30-34 */
enum NTTType { Standard = 0, Coset = 1 };                    /* lib.rs:36-40 */

/* ---------------------------------------------------------------------------------------------
 * Part 1 - the reference's FFI
 * ------------------------------------------------------------------------------------------- */

/* lib.rs:43-49 / snarkvm_api.cu:53-62.  In-place NTT of 2^lg_domain_size Fr elements (32 B each,
 * Montgomery form, host memory).  NN/Forward/Standard == EvaluationDomain::fft_in_place;
 * Inverse includes the 1/n scaling; Forward+Coset multiplies x[j] by 22^j first; Inverse+Coset
 * multiplies the result by 22^-j (fft/domain.rs:201-206, 403-443).  Domains up to 2^28 (the SRS maximum);
 * lg_domain_size > 28 returns hipErrorMemoryAllocation (the caller then uses its CPU path), and so does a
 * device allocation that fails. */
RustError snarkvm_ntt(void *inout, uint32_t lg_domain_size, enum NTTInputOutputOrder ntt_order,
                      enum NTTDirection ntt_direction, enum NTTType ntt_type);

/* lib.rs:51-60 / snarkvm_api.cu:64-75.  Product of `pcount` coefficient-form polynomials and
 * `ecount` evaluation-form vectors over the 2^lg_domain_size domain (PolyMultiplier::multiply,
 * fft/polynomial/multiplier.rs:70-134).  `polynomials` / `evaluations` are arrays of pointers to Fr
 * vectors, `plens` / `elens` their lengths (size_t); every elens[i] must equal the domain size.
 * `out` holds 2^lg_domain_size elements.  Corner cases follow snarkvm.cu:196-210.  lg_domain_size <= 28, as for snarkvm_ntt; the
 * device holds four vectors of the domain (8 GiB each at 2^28). */
RustError snarkvm_polymul(void *out, size_t pcount, const void *polynomials, const void *plens, size_t ecount,
                          const void *evaluations, const void *elens, uint32_t lg_domain_size);

/* lib.rs:62-68 / snarkvm_api.cu:77-83.  out (G1Projective: Jacobian X, Y, Z, 3 x 48 B Montgomery)
 * = sum_i scalars[i] * points[i].  `points_with_infinity` is a Rust `[G1Affine]` (x, y, infinity flag;
 * stride `ffi_affine_sz` = 104 bytes), `scalars` are npoints canonical 256-bit integers < r. */
RustError snarkvm_msm(void *out, const void *points_with_infinity, size_t npoints, const void *scalars,
                      size_t ffi_affine_sz);
/* Multi-GPU: like the reference (snarkvm.cu:254-295) a call of >= 2^19 pairs is cut into point-range chunks that are dealt
 * to every selected device (and to two lanes per device, so that the upload of one chunk overlaps the computation of the
 * previous one); the per-chunk partial results are combined on the host.
 * Ownership: like the reference's symbol the call is STATELESS - `points_with_infinity` and `scalars` are only read during the
 * call and nothing about them is retained after return.
 * Opt-in extension (off unless SNARKVM_HIP_BASE_CACHE is set in the environment): a host base range passed a SECOND
 * time with the same address and length is kept in HBM (converted, with precomputed tables - 17 x 15-bit below 2^18 points,
 * 16 x 16, 13 x 20 from 2^21, 12 x 22 from 2^24 - on every device) and later calls whose bases are a slice of it skip upload
 * and conversion - the reference's callers always pass slices of one long-lived `powers_of_beta_g` vector
 * (kzg10/mod.rs:117-119).  Host memory is only read inside the slice the current call passed.  Two modes:
 *  - sampled (SNARKVM_HIP_BASE_CACHE=1/2/4/8/16): by setting the variable the caller promises that such vectors are immutable
 *    while the process uses them (a hit is verified against raw copies of every 64th point of the slice, which cannot catch
 *    every mutation);
 *  - verified (SNARKVM_HIP_BASE_CACHE=verified, the 16-table geometry, or verified:1/2/4/8/16): the registering call also
 *    copies the 97 payload bytes of every point (x, y, infinity flag; never the padding) into a host shadow, and every hit
 *    compares all npoints x 97 bytes of its slice with it on a small host pool (SNARKVM_HIP_VERIFY_THREADS, default 4, 1..16)
 *    while the device computes; on any difference the entry is dropped and the call is computed stateless, so the result
 *    always reflects the bytes passed in and the caller promises nothing.  SNARKVM_HIP_BASE_CACHE_HOST_MB caps the shadow
 *    bytes (default 4096).
 * SNARKVM_HIP_BASE_CACHE_MB caps the HBM bytes per device (default 65536); least recently used ranges go first.  Switching
 * between the modes drops every cached range.  Code that can be changed should call snarkvm_hip_register_bases* +
 * snarkvm_hip_msm_registered*.
 * snarkvm_hip_set_base_cache(tables) / snarkvm_hip_set_base_cache_verified(tables) are the API forms of the variable (0, 1, 2, 4, 8 or
 * 16; they override the environment from then on and need no device; 0 means off and also drops every cached range) - for a host
 * that cannot set the environment before the library is loaded. */
RustError snarkvm_hip_set_base_cache(int tables);
RustError snarkvm_hip_set_base_cache_verified(int tables);
/* What the base cache of snarkvm_msm did since the last reset: out[8] = {lookups, hits (results served from the cached tables; in
 * verified mode only after the comparison agreed), registrations, verification mismatches, bytes compared, microseconds callers
 * waited for their comparison after their device result was ready, tables in effect (0: off), verified mode (0 / 1)}; reset != 0
 * clears the first six. */
void snarkvm_hip_base_cache_stats(uint64_t *out, int reset);

/* ---------------------------------------------------------------------------------------------
 * Part 2 - extension ABI (device-resident data, SRS registration, instrumentation)
 * ------------------------------------------------------------------------------------------- */

/* Number of visible HIP devices (0 if none).  Never fails. */
int snarkvm_hip_device_count(void);
/* Number of HIP streams (each with its own workspace) snarkvm_hip_msm_registered_batch cycles through for instances of
 * up to `npoints` pairs: 8 below 2^20, 3 above (SNARKVM_HIP_TUNING=lanes=N overrides).  A caller that wants allocation-free timed
 * regions warms up that many instances first (snarkvm_hip_alloc_stats tells whether anything grew). */
int snarkvm_hip_batch_lanes(size_t npoints);
/* Devices used by this process (the reference loops over `ngpus()`, snarkvm.cu:123-151).  Default: every visible device, or
 * the comma-separated list in SNARKVM_HIP_DEVICES.  snarkvm_hip_set_devices selects them explicitly; it must be called before
 * the first compute call (afterwards only the identical list is accepted).  An id may be listed more than once: each entry
 * is an independent logical device (own streams, workspaces, base replicas) - how the multi-device paths are tested on a
 * one-GPU box.  snarkvm_hip_set_device(d) == set_devices({d}): the one-process-per-GPU deployment (LOCAL_RANK mapping is the
 * caller's business).  snarkvm_hip_num_devices: logical devices in use (0 if none can be initialised). */
RustError snarkvm_hip_set_devices(const int32_t *ids, size_t n);
RustError snarkvm_hip_set_device(int device);
int snarkvm_hip_num_devices(void);

/* Device memory for a host that has no HIP binding of its own (a Rust prover that keeps its polynomials in HBM between the transforms
 * and the commitments; the reference's plugin owns every device byte itself, snarkvm.cu:51,123-151): what the device-resident entry
 * points below take as `d_*` pointers.  `device` of snarkvm_hip_malloc: index into the devices in use (snarkvm_hip_set_devices), or -1 =
 * the device of the calling thread's open scope, logical device 0 outside a scope.  Blocks are NOT counted by snarkvm_hip_alloc_stats (that
 * reports the library's own workspace growth).  snarkvm_hip_free waits for all queued work of the device first (hipFree).
 * Copies with a HOST side (h2d, d2h) return when the copy is complete: `src` may be reused, `dst` may be read.  Inside a scope of the
 * calling thread they are ordered behind the work the scope has queued on its stream (and wait for that, not for the scope's enqueued MSMs).
 * snarkvm_hip_memcpy_d2d and snarkvm_hip_memset are device-side operations like the snarkvm_hip_fr_* kernels: inside a scope they are only
 * enqueued on the scope's stream, in call order ("the prover produced a polynomial"); outside a scope they return when done.  d2d ranges
 * must not overlap; the two pointers may live on different devices in use. */
RustError snarkvm_hip_malloc(void **d_ptr, size_t bytes, int device);
RustError snarkvm_hip_free(void *d_ptr);
RustError snarkvm_hip_memcpy_h2d(void *d_dst, const void *src, size_t bytes);
RustError snarkvm_hip_memcpy_d2h(void *dst, const void *d_src, size_t bytes);
RustError snarkvm_hip_memcpy_d2d(void *d_dst, const void *d_src, size_t bytes);
RustError snarkvm_hip_memset(void *d_dst, int value, size_t bytes);

/* Same as snarkvm_ntt but `d_inout` is device memory (the call runs on the device that owns it).  lg_domain_size <= 28. */
RustError snarkvm_hip_ntt_device(void *d_inout, uint32_t lg_domain_size, int ntt_order, int ntt_direction,
                                 int ntt_type);
/* `count` independent in-place transforms of 2^lg_domain_size elements over device vectors on one device: one enqueue, ONE
 * synchronisation (the iNTTs of a prover round, e.g. z_a, z_b, z_c: algorithms/src/snark/varuna/ahp/prover/round_functions/
 * second.rs:104-113).  ntt_directions / ntt_types: one value per vector, or NULL for all forward / all standard.  A vector
 * listed twice is transformed twice, in list order.  Consecutive distinct vectors with the same direction and type share ONE
 * kernel launch per pass (up to 48 vectors; 24 at 2^27 and 12 at 2^28, so that the scratch stays within 48 vectors of 2^26).
 * lg_domain_size <= 28. */
RustError snarkvm_hip_ntt_device_batch(void *const *d_inouts, size_t count, uint32_t lg_domain_size, int ntt_order,
                                       const int *ntt_directions, const int *ntt_types);

/* snarkvm_polymul over operands that live in device memory and stay there: d_out (2^lg_domain_size elements) = the product of `pcount`
 * coefficient-form polynomials d_polys[k] of plens[k] elements and `ecount` evaluation-form vectors d_evals[k] (natural order over the
 * domain, elens[k] == 2^lg_domain_size), reduced mod X^n - 1 like the host symbol.  d_polys / d_evals are HOST arrays of device pointers,
 * read during the call and not retained.  Nothing is staged: the forward transforms read each polynomial where it is (zero beyond its
 * length), the inverse transform reads the product of the evaluation-form factors, and no pointwise pass runs in between.
 *  - Output: with at least one operand all 2^lg_domain_size elements of d_out are written - also for a single polynomial (a copy, then a
 *    zeroed tail; the host symbol leaves that tail to its caller's pre-zeroed buffer, so the two agree whenever that contract is met).
 *  - pcount + ecount == 0: success, nothing is touched, no device is needed.
 *  - Operands are never written.  plens[k] may be anything from 0 to 2^lg_domain_size; a zero-length polynomial makes the product zero.
 *  - d_out may coincide exactly with the START of one operand (v <- v * d in place): every read of that operand is ordered before the
 *    first write of d_out.  Any other overlap of d_out with an operand is refused with hipErrorInvalidValue before anything is launched.
 *  - Errors, none of which leaves a partial result: lg_domain_size > 28 -> hipErrorMemoryAllocation (as snarkvm_ntt); plens[k] >
 *    2^lg_domain_size, elens[k] != 2^lg_domain_size, a null pointer, an operand on another device than d_out -> hipErrorInvalidValue.
 *  - Inside a snarkvm_hip_scope the call is only enqueued, in order with the other device-resident calls.
 *  - Workspace (from the calling lane; a repeated call grows nothing, snarkvm_hip_alloc_stats), in vectors of 2^lg_domain_size elements:
 *    pcount == 0: 1.  Otherwise r + 1 with r = min(pcount, 48, 48 * 2^26 / 2^lg_domain_size) - the coefficient operands are transformed r at
 *    a time, one kernel launch per pass but the last, which runs per operand so that the results can reuse the slots it frees: 3 vectors
 *    for two polynomials.  One more vector (an accumulator) when pcount > r, or when more than 4 evaluation-form factors remain
 *    ((pcount - 1) mod r + 1 transforms of the last chunk, the accumulator, ecount): those are multiplied 4 at a time.
 *    At lg_domain_size == 0: 1, plus the accumulator beyond 4 operands. */
RustError snarkvm_hip_polymul_device(void *d_out, size_t pcount, const void *const *d_polys, const size_t *plens, size_t ecount,
                                     const void *const *d_evals, const size_t *elens, uint32_t lg_domain_size);

/* Deferred synchronisation for device-resident operands.  Between snarkvm_hip_scope_begin (d_any: any device pointer on the GPU
 * to use, or NULL for any GPU) and snarkvm_hip_scope_end, calls of THIS thread whose operands and results live in device memory
 * - snarkvm_hip_ntt_device, _ntt_device_batch, _polymul_device, _fr_mul_device, _fr_convert_device, _memcpy_d2d, _memset and the snarkvm_hip_fr_* vector
 * kernels (snarkvm_hip_fr_lincomb and snarkvm_hip_fr_spmv among them) with on_device = 1 - are enqueued on one stream, in call order, and return without waiting; snarkvm_hip_scope_end waits once.  The
 * 32-byte host `remainder` of snarkvm_hip_fr_divide_by_linear with on_device = 1 is delivered by scope_end, and so are the host results of
 * snarkvm_hip_fr_reduce[_strided], snarkvm_hip_fr_evaluate, snarkvm_hip_fr_support[_strided] and the counts of snarkvm_hip_fr_rowcheck_fold over device operands (the same mechanism: parked in pinned memory, copied
 * to the caller's buffer when the scope is flushed - the buffer must stay valid until then).  Every other call (MSMs,
 * host buffers, a pointer on another GPU) first waits for the scope's queued work, so results are the same as without a scope - and
 * then runs on the scope's own stream: a thread inside a scope never waits for a free stream.  Scopes do not nest; a scope must be
 * ended by the thread that began it (a thread that ENDS with its scope still open returns the scope's streams to the pool: the queued work is
 * waited for, results it still owed are dropped). */
RustError snarkvm_hip_scope_begin(const void *d_any);
RustError snarkvm_hip_scope_end(void);
/* The same with options.  SNARKVM_HIP_SCOPE_ASYNC_MSM: snarkvm_hip_msm_registered[_ex / _batch / _batch_ex] and
 * snarkvm_hip_msm_g2_registered[_batch] calls of this thread whose scalars live in the scope's GPU memory are ENQUEUED too (on further
 * streams of the scope, behind everything the scope has been given so far) and return at once: their `out` buffers are written by
 * snarkvm_hip_scope_end - or by any call that has to wait for the scope - and must stay valid until then; the scalar vectors may be
 * overwritten by later calls of the scope (those wait on the GPU until the MSM has read them).  How one prover thread keeps the GPU
 * busy across the rounds of a proof: the commitments of round k run beside the transforms of round k + 1 and their host finishes run
 * while the GPU works (the reference's rayon workers overlap the same way on the CPU, polycommit/sonic_pc/mod.rs:186-245).
 * SNARKVM_HIP_SCOPE_STABLE_INPUTS (with ASYNC_MSM): the caller promises not to touch the scalar vectors of its enqueued MSMs before the
 * scope ends; the scope's stream then never waits for an MSM (without the flag every later call of the scope waits, on the GPU, until
 * the MSM has read its scalars - which an MSM queued behind others does late).
 * A thread holds at most 1 + 7 streams per scope and a GPU lends at most 12 of its 16 streams to scopes: a scope_begin beyond that waits,
 * and a scope that finds no further stream free runs its MSMs on the streams it has.
 * snarkvm_hip_scope_stream: the hipStream_t the scope's device-resident calls are enqueued on (NULL outside a scope) - a caller that
 * produces operands with its own kernels or copies (hipMemcpyAsync, torch.cuda.ExternalStream) orders them with the scope's calls by
 * using this stream.
 * SNARKVM_HIP_SCOPE_MSM_IN_STREAM (with ASYNC_MSM): the MSMs are enqueued on the scope's OWN stream, in order with its transforms, instead of
 * a further stream - no hand-off between streams; for the MSMs a caller collects (snarkvm_hip_scope_collect) before it issues anything else,
 * beside which nothing could run anyway.  snarkvm_hip_scope_set_flags changes the flags of the open scope for the calls that follow: a prover
 * enqueues its independent MSM (G2) on a further stream first and then runs the transcript-ordered commitment rounds in-stream, each
 * collected before the next round's challenge is drawn, with the independent MSM filling the gaps. */
enum { SNARKVM_HIP_SCOPE_ASYNC_MSM = 1, SNARKVM_HIP_SCOPE_STABLE_INPUTS = 2, SNARKVM_HIP_SCOPE_MSM_IN_STREAM = 4 };
/* snarkvm_hip_scope_collect(out): waits until the MSM call that was given `out` as its (first) output buffer is done and writes its outputs
 * (out == NULL: every MSM this thread's scope has enqueued so far); the scope stays open, the work queued on its own stream is NOT waited for
 * and the other enqueued MSMs stay pending - except that outputs of other MSMs whose results have ALREADY arrived may be written too while this
 * call would only wait (their `out` buffers are owed by scope_end at the latest; this moves their host finish off the end of the scope).
 * What a prover needs between two rounds: the commitments of round k
 * go into the Fiat-Shamir transcript before the challenge of round k + 1 exists (snark/varuna/varuna.rs:336 ff.), while transforms that do
 * not depend on that challenge - and the tails of earlier MSMs, and an independent MSM - keep running. */
RustError snarkvm_hip_scope_begin_ex(const void *d_any, uint32_t flags);
RustError snarkvm_hip_scope_collect(const void *out);
RustError snarkvm_hip_scope_set_flags(uint32_t flags);
void *snarkvm_hip_scope_stream(void);

/* Register a base vector once (SRS powers are static per proving key; the reference re-uploads
 * 104 B/point on every call, snarkvm.cu:262-275).  `points` is a Rust `[G1Affine]` with the given
 * stride, in host (on_device = 0) or device (on_device = 1) memory.  Every selected device receives its own replica
 * (host source: parallel uploads; device source: peer copies of the finished tables).  Returns an opaque handle. */
typedef struct snarkvm_hip_bases snarkvm_hip_bases_t;
RustError snarkvm_hip_register_bases(snarkvm_hip_bases_t **handle, const void *points, size_t npoints,
                                     size_t ffi_affine_sz, int on_device);
/* Same, additionally precomputing `tables` (1, 2, 4, 8 or 16) multiples 2^(256/tables * j) * P_i of every base
 * (one-time cost; tables x 96 B per point of HBM).  An MSM over such a handle needs only 256/(tables*c) bucket
 * windows: the serial Horner tail and the bucket reduction shrink by `tables` while the result stays the same
 * group element. */
RustError snarkvm_hip_register_bases_tables(snarkvm_hip_bases_t **handle, const void *points, size_t npoints,
                                            size_t ffi_affine_sz, int on_device, int tables);
/* General form: table j = 2^(window_bits * j) * P_i for j < tables, with tables * window_bits >= 254 and window_bits <= 23.
 * With window_bits > 16 a large MSM runs ONE bucket window of 2^(window_bits - 1) buckets: only `tables` bucket additions
 * per scalar (12 at window_bits = 22 instead of 16) at the price of a deeper sort and a two-axis bucket fold - the
 * Pippenger optimum for n ~ 2^24.  Smaller MSMs over the same handle fall back to a divisor of window_bits. */
RustError snarkvm_hip_register_bases_windowed(snarkvm_hip_bases_t **handle, const void *points, size_t npoints,
                                              size_t ffi_affine_sz, int on_device, int tables, int window_bits);
void snarkvm_hip_free_bases(snarkvm_hip_bases_t *handle);

/* The reference's canonical encoding of G1 points (curves/src/templates/macros.rs:66-140, utilities/src/serialize/
 * flags.rs:72-99) decoded / encoded on the device: uncompressed = x, y as 48-byte little-endian canonical integers with
 * the infinity flag in bit 6 of the last byte (96 B; the body of a `.usrs` SRS file after its u64 count); compressed =
 * x with bit 7 = "y is the larger root", bit 6 = infinity (48 B; y recovered by a square root, affine.rs:140-150).
 * validate = 1 additionally checks curve and prime-order-subgroup membership (`Valid::check`, macros.rs:106-113).
 * Errors (both flag bits set, coordinate >= q, no square root, failed validation) return a non-zero code and name the
 * SerializationError in the message.
 * register_bases_serialized: bytes (host) -> a registered base vector, never materialising the Rust layout. */
RustError snarkvm_hip_register_bases_serialized(snarkvm_hip_bases_t **handle, const void *bytes, size_t npoints,
                                                int compressed, int validate, int tables);
/* bytes (host) -> Rust `[G1Affine]` (104 B stride, host) and back. */
RustError snarkvm_hip_g1_deserialize(void *out_affine, const void *bytes, size_t n, int compressed, int validate);
RustError snarkvm_hip_g1_serialize(void *out_bytes, const void *affine, size_t n, size_t ffi_affine_sz, int compressed);

/* G2 points, uncompressed (192 B: x.c0, x.c1, y.c0, y.c1 canonical little-endian, flags in the last byte; fp2.rs:425-455),
 * e.g. `beta-h.usrs`: bytes (host) <-> Rust `[G2Affine]` (200 B stride, host). */
RustError snarkvm_hip_g2_deserialize(void *out_affine, const void *bytes, size_t n, int validate);
RustError snarkvm_hip_g2_serialize(void *out_bytes, const void *affine, size_t n, size_t ffi_affine_sz);
/* Compressed G2 points (96 B: x.c0, x.c1 with the flags; y = `Fp2::sqrt` of x^3 + b' selected by the sign flag in the order
 * of fields/src/fp2.rs:240-250, all on the device; fields/src/fp2.rs:208-230, curves/src/templates/.../affine.rs:140-150). */
RustError snarkvm_hip_g2_deserialize_compressed(void *out_affine, const void *bytes, size_t n, int validate);
RustError snarkvm_hip_g2_serialize_compressed(void *out_bytes, const void *affine, size_t n, size_t ffi_affine_sz);

/* MSM over registered bases [offset, offset + npoints).  `scalars` in host (scalars_on_device = 0) or
 * device memory.  `out` is a 144-byte host buffer (Jacobian, as snarkvm_msm).  `window_bits` = 0 picks
 * the window size automatically. */
RustError snarkvm_hip_msm_registered(void *out, const snarkvm_hip_bases_t *handle, size_t offset, size_t npoints,
                                     const void *scalars, int scalars_on_device, int window_bits);

/* KZG10-shaped MSM over registered bases: sum over two base ranges [off0, off0+n0) and [off1, off1+n1) with
 * n0 + n1 consecutive scalars - the plaintext MSM and the hiding MSM of KZG10::commit
 * (polycommit/kzg10/mod.rs:119,149) in one launch.  scalars_montgomery = 1 fuses `convert_to_bigints`
 * (kzg10/mod.rs:469-474: Fr::to_bigint per coefficient) into the scalar-read phase. */
RustError snarkvm_hip_msm_registered_ex(void *out, const snarkvm_hip_bases_t *handle, size_t off0, size_t n0,
                                        size_t off1, size_t n1, const void *scalars, int scalars_on_device,
                                        int scalars_montgomery, int window_bits);

/* A batch of independent MSMs over one registered base vector (the commitments of a batch of proofs,
 * polycommit/sonic_pc/mod.rs:186-245 fans these out over a CPU pool).  Instance k covers bases
 * [offsets[k], offsets[k] + npoints[k]) with the scalar vector scalars[k]; results are written to
 * outs + 144 * k.  Instances are dealt to the selected devices (host scalars: round-robin; device scalars: the device that
 * owns them) and, on each device, pipelined over several HIP streams so that the latency-bound tail of one MSM overlaps
 * the accumulation of the next. */
RustError snarkvm_hip_msm_registered_batch(void *outs, const snarkvm_hip_bases_t *handle, size_t count,
                                           const size_t *offsets, const size_t *npoints, const void *const *scalars,
                                           int scalars_on_device, int scalars_montgomery, int window_bits);

/* The same with two base ranges per instance: bases [off0[k], off0[k] + n0[k]) followed by [off1[k], off1[k] + n1[k]) against
 * n0[k] + n1[k] consecutive scalars - a whole round of KZG10 commitments (plaintext + hiding MSM each, polycommit/kzg10/
 * mod.rs:119,149; degree-bounded ones start at a shifted-powers offset, sonic_pc/mod.rs:203-245) in one call. */
RustError snarkvm_hip_msm_registered_batch_ex(void *outs, const snarkvm_hip_bases_t *handle, size_t count, const size_t *off0,
                                              const size_t *n0, const size_t *off1, const size_t *n1,
                                              const void *const *scalars, int scalars_on_device, int scalars_montgomery,
                                              int window_bits);

/* out (144 B) = sum of n G1Projective points (host buffers).  Combines the per-device partial results of an MSM whose
 * point range was split over several GPUs (the host `dadd` loop of snarkvm.cu:290-295). */
RustError snarkvm_hip_g1_sum(void *out, const void *in_projective, size_t n);

/* `From<Projective> for Affine` (curves/src/templates/short_weierstrass_jacobian/affine.rs:331-353) for n
 * G1Projective (144 B) -> G1Affine (104 B), host buffers. */
RustError snarkvm_hip_g1_to_affine(void *out_affine, const void *in_projective, size_t n);

/* G2 variable-base MSM (the reference routes G2 through its CPU `standard::msm`,
 * msm/variable_base/{mod.rs:45-47,standard.rs:79-105}; north_star asks for it on the device).
 * `points_with_infinity` is a Rust `[G2Affine]` (x, y in Fq2 = 96 B each, infinity flag; stride 200 B);
 * `out` is a G2Projective (Jacobian, 288 B). */
RustError snarkvm_hip_msm_g2(void *out, const void *points_with_infinity, size_t npoints, const void *scalars,
                             size_t ffi_affine_sz);

/* Registered G2 bases (static G2 vectors, e.g. powers of beta H): the same precomputed-table scheme as
 * snarkvm_hip_register_bases_tables / _windowed (window_bits = 0: tables in {1, 2, 4, 8, 16} of 256 / tables bits).  Without
 * tables a G2 MSM ends in a serial chain of ~240 Fq2 doublings (~10 ms whatever its size); with them that chain is gone.
 * `points` is a host Rust `[G2Affine]` (stride >= 200), `out` a G2Projective (288 B). */
typedef struct snarkvm_hip_bases_g2 snarkvm_hip_bases_g2_t;
RustError snarkvm_hip_register_bases_g2(snarkvm_hip_bases_g2_t **handle, const void *points, size_t npoints,
                                        size_t ffi_affine_sz, int tables, int window_bits);
void snarkvm_hip_free_bases_g2(snarkvm_hip_bases_g2_t *handle);
RustError snarkvm_hip_msm_g2_registered(void *out, const snarkvm_hip_bases_g2_t *handle, size_t offset, size_t npoints,
                                        const void *scalars, int scalars_on_device, int window_bits);
/* A batch of independent G2 MSMs over one registered vector, fanned out over devices and lanes like
 * snarkvm_hip_msm_registered_batch; results are written to outs + 288 * k. */
RustError snarkvm_hip_msm_g2_registered_batch(void *outs, const snarkvm_hip_bases_g2_t *handle, size_t count,
                                              const size_t *offsets, const size_t *npoints, const void *const *scalars,
                                              int scalars_on_device, int window_bits);

/* Setup-time group operations.  Host buffers.
 * fixed_base_msm: out[i] (G1Projective, 144 B) = scalars[i] * g for one base `g` (Rust G1Affine, 104 B) and n Fr
 *   scalars in Montgomery form - FixedBase::msm (msm/fixed_base.rs:33-97; the window table is built on the device).
 * group_ntt: in-place radix-2 transform of 2^lg G1Projective points with Fr twiddles; inverse = 1 includes the 1/n
 *   scaling - `EvaluationDomain::ifft` over group elements as used by UniversalParams::lagrange_basis
 *   (polycommit/kzg10/data_structures.rs:68-72).  Results are group elements: compare after to_affine. */
RustError snarkvm_hip_g1_fixed_base_msm(void *out_projective, const void *g_affine, const void *scalars, size_t n);
RustError snarkvm_hip_g1_group_ntt(void *inout_projective, uint32_t lg_domain_size, int inverse);

/* Fr vector helpers on device memory: out[i] = a[i] * b[i] (polynomial_inner_multiply,
 * polynomial.cuh:36-45); Fr::to_bigint / from_bigint over a vector (kzg10/mod.rs:469-474). */
RustError snarkvm_hip_fr_mul_device(void *d_out, const void *d_a, const void *d_b, size_t n);
RustError snarkvm_hip_fr_convert_device(void *d_out, const void *d_in, size_t n, int to_bigint);

/* Prover-round Fr vector kernels: the O(n) passes the Varuna prover runs between its NTTs and commitments
 * (SURVEY.md 8f N2, and the `open` half of KZG10).  Vectors are Fr elements in the reference's memory form
 * (32 B, Montgomery); with on_device = 1 every vector pointer is device memory on the context's device, otherwise host
 * memory (staged through HBM by the call).  Scalar operands (`scalar`, `point`, `coeff`, `g`, `c`, `tau`) and the
 * `remainder` of divide_by_linear are always 32-byte HOST values.
 *
 * fr_vec_op: op 0 out = a + b | 1 a - b | 2 a * b | 3 a * b - c (round_functions/second.rs:110-111: rowcheck)
 *            | 4 a * scalar | 5 a - scalar (kzg10/mod.rs:295) | 6 a + b * scalar (second.rs:113) | 7 scalar - a. */
RustError snarkvm_hip_fr_vec_op(int op, void *out, const void *a, const void *b, const void *c, const void *scalar,
                                size_t n, int on_device);
/* `polynomial / (X - point)` and `polynomial.evaluate(point)` in one pass (KZG10::compute_witness_polynomial,
 * kzg10/mod.rs:213-236 via polynomial/mod.rs:222-256; DensePolynomial::evaluate, dense.rs:98-114): quotient gets
 * n - 1 coefficients (may be NULL when only the value is wanted), *remainder = p(point).  With on_device = 1 `quotient` must not
 * overlap `poly` (coefficient ranges are owned by different workgroups: an in-place division would race); such a call is refused. */
RustError snarkvm_hip_fr_divide_by_linear(void *quotient, void *remainder, const void *poly, size_t n,
                                          const void *point, int on_device);
/* batch_inversion_and_mul (fields/src/lib.rs:66-129): v_i <- coeff / v_i, zero elements stay zero. */
RustError snarkvm_hip_fr_batch_inversion_and_mul(void *inout, size_t n, const void *coeff, int on_device);
/* EvaluationDomain::distribute_powers_and_mul_by_const (fft/domain.rs:224-254): v_i <- v_i * c * g^i. */
RustError snarkvm_hip_fr_distribute_powers(void *inout, size_t n, const void *g, const void *c, int on_device);
/* EvaluationDomain::evaluate_all_lagrange_coefficients (fft/domain.rs:258-292) for the 2^lg domain. */
RustError snarkvm_hip_fr_lagrange_coefficients(void *out, uint32_t lg_domain_size, const void *tau, int on_device);
/* DensePolynomial::divide_by_vanishing_poly (dense.rs:161-169): division of `len` coefficients by X^domain_size - 1.
 * quotient: len - domain_size coefficients (untouched when len <= domain_size); remainder: min(len, domain_size). */
RustError snarkvm_hip_fr_divide_by_vanishing(void *quotient, void *remainder, const void *poly, size_t len,
                                             size_t domain_size, int on_device);
/* DensePolynomial::mul_by_vanishing_poly (dense.rs:153-159): out (len + domain_size coefficients) = p * (X^D - 1). */
RustError snarkvm_hip_fr_mul_by_vanishing(void *out, const void *poly, size_t len, size_t domain_size, int on_device);

/* Linear combination of polynomials in one pass: out[i] = sum_k coeffs[k] * polys[k][i] for i < n_out, polys[k][i] counting as zero from
 * lens[k] on - every linear combination SonicKZG10::open_combinations materialises (`poly += (coeff, cur_poly)` per term,
 * polycommit/sonic_pc/mod.rs:413-473) and the fold of batch_open (combine_polynomials, mod.rs:548-564).  Followed by
 * snarkvm_hip_fr_divide_by_linear over `out` the remainder is the combination's evaluation (get_lc_eval, snark/varuna/varuna.rs:584-590).
 * `polys`, `lens` and `coeffs` (count x 32 bytes, Montgomery form) are HOST arrays, read during the call and not retained; on_device
 * governs `out` and every polys[k].  A pointer may be NULL iff its length is 0.  The device reads K + 1 vectors where a chain of
 * fr_vec_op calls moves 3K - 1; operands travel 24 per kernel launch (FR_LINCOMB_CHUNK), a longer list takes `out` back in as a term.
 *  - Output: all n_out elements are written, zeros past the longest operand; count == 0 zero-fills.
 *  - n_out == 0: success, nothing is touched, no device is needed.
 *  - `out` may coincide exactly with the START of one operand (p <- p + sum ...): that operand is read before `out` is written.  Any other
 *    overlap of `out` with an operand is refused with hipErrorInvalidValue before anything is launched (so is `out` listed as an operand
 *    more than 24 times).  Operands may overlap each other and repeat; they are never written.
 *  - Errors, none of which leaves a partial result: lens[k] > n_out, a missing pointer, an operand on another device than `out`
 *    -> hipErrorInvalidValue.
 *  - With on_device = 1 inside a snarkvm_hip_scope the call is only enqueued.
 *  - With on_device = 0 the operands are staged into one lane buffer (n_out + sum lens[k] elements): one upload each, one download.
 *  - Workspace: none with on_device = 1; a repeated call grows nothing (snarkvm_hip_alloc_stats). */
RustError snarkvm_hip_fr_lincomb(void *out, size_t n_out, size_t count, const void *const *polys, const size_t *lens, const void *coeffs,
                                 int on_device);

/* Opening fold: a linear combination of polynomials, its quotient by X - point and its value at `point` in one sweep up and one sweep down -
 * the polynomial side of one query point of SonicKZG10::open_combinations / batch_open (polycommit/sonic_pc/mod.rs:286-342, 413-473 into
 * KZG10::compute_witness_polynomial, kzg10/mod.rs:213-236) once the opening challenges have been folded into the coefficients on the host
 * (sum_lc xi_lc sum_k a_(lc,k) p_k = sum_k (sum_lc xi_lc a_(lc,k)) p_k), and with quotient = NULL the get_lc_eval of snark/varuna/varuna.rs:583-590.
 *    comb[i] = sum_k coeffs[k] * polys[k][i]  for i < n, polys[k][i] counting as zero from lens[k] on
 *    h_i     = sum_{j >= i} comb[j] * point^(j - i)
 *  - quotient (optional): a buffer of n elements, ALL written: quotient[i] = h_(i+1).  The first n - 1 elements are the coefficients of
 *    comb / (X - point); quotient[n - 1] = h_n = 0.
 *  - remainder (optional): a 32-byte HOST value, h_0 = comb(point).
 * `polys`, `lens`, `coeffs` (count x 32 bytes, Montgomery form) and `point` are HOST arrays, read during the call and not retained; on_device
 * governs `quotient` and every polys[k], as in snarkvm_hip_fr_lincomb.  A pointer may be NULL iff its length is 0.
 * The combination is formed once and parked in quotient[i]; the up sweep folds it into block values, the down sweep replaces it by h_(i+1)
 * in place (every thread writes only the indices it has just read).  Against snarkvm_hip_fr_lincomb per combination, one more to fold them and
 * snarkvm_hip_fr_divide_by_linear - L + 4 launches, K + 2L + 4 vector passes, L + 1 intermediate vectors, (K + L + 2) n products for L
 * combinations over K members - a single member is combined inside the sweep: 3 launches, 4 passes, 3 n products.  A thread of the sweep
 * reads its own run of consecutive coefficients, which does not coalesce, so of two or more members all go through accumulating fr_lincomb
 * launches into the quotient buffer first (24 per launch, FR_LINCOMB_CHUNK; measured faster at every shape than forming the combination
 * inside the sweep, profiles/fr_open_fold.md) and the sweep finds the combination parked there: 4 launches up to K = 24, K + 4 passes,
 * (K + 2) n products, still no vector beside the quotient.  Without a quotient there is no buffer to accumulate in: every table of 24
 * members gets an up sweep of its own and the values are added.  The route is the one
 * snarkvm_hip_fr_divide_by_linear takes for n: three launches with a scan inside every workgroup for 2048 <= n <= 2^20 and a quotient, the
 * chunk recursion otherwise.  No atomics, a fixed order of additions: the bytes do not depend on the launch geometry.
 *  - n == 0: success, a given remainder is set to zero, nothing else is touched, no device is needed.
 *  - count == 0, or every lens[k] == 0: the quotient is zero-filled, the remainder is zero.
 *  - Refused with hipErrorInvalidValue before anything is launched, no partial result: lens[k] > n; a missing pointer with a non-zero length;
 *    a missing `point`; missing `coeffs`, `polys` or `lens` with count > 0; an operand on another device than `quotient`; `quotient`
 *    overlapping any operand, its own start included (no in-place form: the quotient buffer is the pass's only workspace).  Operands may
 *    overlap each other and repeat; they are never written.
 *  - With on_device = 1 inside a snarkvm_hip_scope the call is only enqueued and the remainder is delivered by snarkvm_hip_scope_end, like
 *    that of snarkvm_hip_fr_divide_by_linear.
 *  - With on_device = 0 the operands are staged into one lane buffer (n + sum lens[k] elements): one upload each, one download.
 *  - Workspace: the lane's scratch for block values only; a repeated call grows nothing (snarkvm_hip_alloc_stats). */
RustError snarkvm_hip_fr_open_fold(void *quotient, void *remainder, size_t n, size_t count, const void *const *polys, const size_t *lens,
                                   const void *coeffs, const void *point, int on_device);

/* Selector fold: the sums of Varuna's round 3 (calculate_lineval_sumcheck_witness, snark/varuna/ahp/prover/round_functions/third.rs:126-327) in
 * one pass.  Member k is a polynomial polys[k] of L_k = lens[k] coefficients, a source domain of n_k = src_sizes[k] elements and a multiplier
 * mu_k = multipliers[k] (combiner * n_k / N).  apply_randomized_selector (ahp/selectors.rs:100-121) scales the member, divides it by X^n_k - 1,
 * multiplies the remainder by X^N - 1 and divides by X^n_k - 1 again; the last two steps tile the remainder over N = target_size coefficients
 * (their own remainder is identically zero when n_k divides N), so summed over the members:
 *    h_out[i]  = sum_k mu_k sum_{j >= 1, i + j n_k < L_k} polys[k][i + j n_k]     for i < h_len      (h_1)
 *    xg_out[i] = sum_k mu_k sum_{j >= 0} polys[k][(i mod n_k) + j n_k]            for i < target_size (x g_1; g_1 is xg_out from coefficient 1 on)
 *    sums[k]   = n_k sum_j polys[k][j n_k]   - NOT scaled by mu_k: the sum of the member over its source domain (third.rs:317), no transform needed.
 * `polys`, `lens`, `src_sizes` and `multipliers` (count x 32 bytes, Montgomery form) are HOST arrays, read during the call and not retained;
 * on_device governs h_out, xg_out, sums (count x 32 bytes) and every polys[k].  A member pointer may be NULL iff its length is 0; a member of
 * length 0 contributes nothing and its sum is 0.  Members may overlap each other and repeat; they are never written.
 *  - Each of the three outputs may be NULL, which skips it (h_len is ignored when h_out is NULL, target_size when xg_out is NULL); with all three
 *    NULL a call whose other arguments are valid succeeds and touches nothing.  Of a given output every element is written: all h_len elements of
 *    h_out (zeros past the longest quotient), all target_size of xg_out, all count of sums.  count == 0 zero-fills h_out and xg_out.
 *  - Nothing to write (no output given, or only an h_out with h_len == 0): success, no device is needed.
 *  - Refused with hipErrorInvalidValue before anything is launched and before a device is needed, every output untouched: NULL host arrays with
 *    count > 0; a NULL member of non-zero length; any n_k == 0; xg_out given and target_size == 0, target_size > 2^28 or an n_k that does not divide
 *    target_size; h_out given and h_len < max_k (L_k - n_k); h_len or any L_k above 2^29; count > 65535; any overlap of an output with a member or
 *    with another output; with on_device = 1, pointers on different devices.
 *  - With on_device = 1 inside a snarkvm_hip_scope the call is only enqueued (sums is device memory like the other outputs: nothing is delivered
 *    at snarkvm_hip_scope_end).
 *  - With on_device = 0 outputs and members are staged in one lane buffer: one upload per member, one download per output.
 *  - Members travel 24 per kernel launch (FR_SELECTOR_CHUNK); a longer list takes further launches that add to the outputs.
 *  - No atomics and a fixed order of additions per output element; field addition is exact and results canonical, so the bytes depend on neither
 *    the grid, the split into launches nor the way the members are grouped.
 *  - Workspace: none with on_device = 1; a repeated call grows nothing (snarkvm_hip_alloc_stats). */
RustError snarkvm_hip_fr_selector_fold(void *h_out, size_t h_len, void *xg_out, size_t target_size, void *sums, size_t count,
                                       const void *const *polys, const size_t *lens, const size_t *src_sizes, const void *multipliers,
                                       int on_device);

/* Witness evaluations: the gather of Varuna's round 1 (calculate_w, snark/varuna/ahp/prover/round_functions/first.rs:127-161) between the forward
 * transform of x_poly and the inverse transform that yields w (X^|X| - 1).  With ratio = n / input_size, for k < n:
 *    out[k] = 0                                      when ratio divides k (the input subgroup)
 *    out[k] = w[k - k / ratio - 1] - x_evals[k]      otherwise; w counts as zero from w_len on.
 * on_device governs out, w and x_evals.  All n elements of out are written.  out may coincide EXACTLY with x_evals (in place on the transform of
 * x_poly: a thread reads x_evals[k] before it writes out[k]); w is never written.
 *  - n == 0 (with a valid input_size): success, nothing is touched and no device is needed.
 *  - Refused with hipErrorInvalidValue before anything is launched and before a device is needed, out untouched: input_size == 0; input_size does
 *    not divide n; n > 2^28; w_len > n - input_size; out or x_evals NULL with n > 0; w NULL with w_len > 0; out overlapping x_evals other than
 *    exactly, or overlapping w; with on_device = 1, operands on different devices.
 *  - With on_device = 1 inside a snarkvm_hip_scope the call is only enqueued.
 *  - With on_device = 0 w, x_evals and out are staged in lane buffers: two uploads, one download.
 *  - Workspace: none with on_device = 1. */
RustError snarkvm_hip_fr_witness_evals(void *out, size_t n, const void *w, size_t w_len, const void *x_evals, size_t input_size, int on_device);

/* Assignment evaluations: Varuna's round 1 in lock step.  The vector above plus the evaluations of x_poly is the evaluation vector of the
 * assignment z = w (X^|X| - 1) + x_poly itself (third.rs:236-239): the padded public input on the input subgroup, the private variables elsewhere -
 * the interleaving of EvaluationDomain::reindex_by_subdomain (fft/domain.rs:322-344).  ONE inverse transform of it at |V| = n yields z; its quotient
 * by X^|X| - 1 (snarkvm_hip_fr_divide_by_vanishing) is w and its remainder is x_poly, deg x_poly < |X|: no forward transform, no transform at |X|.
 * `count` members (the instances of one circuit); member m reads the row v = vars + m * stride_vars and writes o = out + m * stride_out, both
 * strides in elements (ignored when count == 1).  A row is  padded_public (input_size values) ++ private (num_vars - input_size values)  - the x
 * operand of snarkvm_hip_fr_spmv for the circuit's matrices.  With ratio = n / input_size, for k < n:
 *    o[k] = v[k / ratio]                                   when ratio divides k
 *    o[k] = v[input_size + (k - k / ratio - 1)]            otherwise; zero where that index is >= num_vars.
 * on_device governs out and vars.  All n elements of every member are written and nothing between the members; vars is never written.  No
 * arithmetic: every element is copied bit for bit.
 *  - count == 0 or n == 0 (arguments otherwise valid): success, nothing is touched and no device is needed.
 *  - Refused with hipErrorInvalidValue before anything is launched and before a device is needed, out untouched: input_size == 0; input_size does
 *    not divide n; n > 2^28; num_vars < input_size or num_vars > n (with n > 0); count > 65535; with count > 1, stride_out < n, stride_vars <
 *    num_vars or a stride of more than 2^40 elements; out or vars NULL with n > 0 and count > 0; out overlapping vars (the spans of all
 *    members); with on_device = 1, operands on different devices.
 *  - With on_device = 1 inside a snarkvm_hip_scope the call is only enqueued.
 *  - With on_device = 0 the rows (as they lie, gaps included) and the outputs are staged in lane buffers: one upload, one download per member.
 *  - One launch: the member on blockIdx.y, up to 8192 workgroups of 256 threads per member (snarkvm_hip_selftest_fr_assignment_geometry).
 *  - Workspace: none with on_device = 1; a repeated call grows nothing (snarkvm_hip_alloc_stats). */
RustError snarkvm_hip_fr_assignment_evals(void *out, size_t n, const void *vars, size_t num_vars, size_t input_size, size_t count, size_t stride_out,
                                          size_t stride_vars, int on_device);

/* Rowcheck fold: the sums of Varuna's round 2 (calculate_rowcheck_witness, round_functions/second.rs:76-142, with apply_randomized_selector
 * without a remainder witness, ahp/selectors.rs:88-99) over `count` members (one per instance of every circuit of one domain size) of three
 * n-element vectors a[k], b[k], c[k] and a multiplier mu_k = multipliers[k]:
 *    out[i]        = sum_k mu_k (a[k][i] b[k][i] - c[k][i])           for i < n
 *    violations[k] = #{ i < n : a[k][i] b[k][i] != c[k][i] }           for k < count
 * Over the evaluations on R the counts are the divisibility test of the round (the remainder by v_R is zero iff every count is); over the
 * evaluations on a coset g R, with mu_k = combiner * |R| / |R_max| / (g^|R| - 1), out holds the coset evaluations of h_0's share of this domain
 * size: one inverse coset transform yields the coefficients.
 * `a`, `b`, `c` (count pointers each), `multipliers` (count x 32 bytes, Montgomery form) and `violations` (count values) are HOST arrays; the
 * first four are read during the call and not retained.  on_device governs out and every a[k], b[k], c[k].  Members may overlap each other and
 * repeat; they are never written.
 *  - Either output may be NULL, which skips it: out NULL is the check alone (multipliers is then ignored and may be NULL), violations NULL the fold
 *    alone; with both NULL a call whose other arguments are valid succeeds and touches nothing.  Of a given output every element is written: all n
 *    of out, all count of violations.  count == 0 zero-fills out.
 *  - n == 0: success, violations is zero-filled, no device is needed.
 *  - Refused with hipErrorInvalidValue before anything is launched and before a device is needed, both outputs untouched: n > 2^28; count > 65535;
 *    a, b or c NULL with count > 0; multipliers NULL with count > 0 and out given; a NULL member pointer with n > 0; any overlap of out with a
 *    member; with on_device = 1, pointers on different devices.
 *  - With on_device = 1 inside a snarkvm_hip_scope the call is only enqueued: out is device memory, violations is delivered by
 *    snarkvm_hip_scope_end (keep it alive until then), like the result of snarkvm_hip_fr_support.
 *  - With on_device = 0 out and the members are staged in one lane buffer: one upload per member vector, one download.
 *  - Members travel 24 per kernel launch (FR_ROWCHECK_CHUNK); a longer list takes further launches: the first writes out, the later ones add to it.
 *  - The Fr output uses no atomics and a fixed order of additions per element; field addition is exact and results canonical, so the bytes depend
 *    on neither the grid, the split into launches nor the way the members are grouped.  The counts are integer sums (one 64-bit integer atomic per
 *    wave that saw a violation): exact whatever the order.
 *  - Workspace: with violations given, count x 8 bytes of the lane's scratch, kept for the next call; a repeated call grows nothing
 *    (snarkvm_hip_alloc_stats). */
RustError snarkvm_hip_fr_rowcheck_fold(void *out, uint64_t *violations, size_t n, size_t count, const void *const *a, const void *const *b,
                                       const void *const *c, const void *multipliers, int on_device);

/* Reductions: a vector -> a value, in one streaming read (csrc/poly.hip.h: fr_reduce_kernel, fr_support_kernel; a second launch folds the
 * per-workgroup partials - no atomics, and since field addition is exact the 32 bytes do not depend on the shape of the tree).
 * fr_reduce: op SNARKVM_HIP_FR_REDUCE_SUM: *result = sum_i a[i] (`b` is ignored; the sum of a polynomial's evaluations over a domain,
 * snark/varuna/ahp/prover/round_functions/first.rs:119); op SNARKVM_HIP_FR_REDUCE_DOT: *result = sum_i a[i] * b[i] - Evaluations::evaluate_with_coeffs
 * (fft/evaluations.rs:90-92) with `b` the vector snarkvm_hip_fr_lagrange_coefficients left in device memory; the products go four at a time
 * through one Montgomery reduction.
 * fr_support: out3 = {trimmed_len, leading_zeros, nonzero}: the index of the last non-zero element + 1 (0 for the zero vector, so that
 * DensePolynomial::degree (dense.rs:88-96) = max(trimmed_len, 1) - 1 and is_zero = trimmed_len == 0), the index of the first non-zero element
 * (n for the zero vector: the count of skip_leading_zeros_and_convert_to_bigints, kzg10/mod.rs:455-467), and the number of non-zero elements.
 *  - Results are HOST values (32 bytes / three uint64_t per vector).  With host operands (on_device = 0: staged like the other passes) they are
 *    there on return.  With device operands inside a snarkvm_hip_scope the call is only enqueued on the scope's stream, in order, and the
 *    values are delivered when the scope is flushed (snarkvm_hip_scope_end), like the `remainder` of snarkvm_hip_fr_divide_by_linear.
 *  - n == 0: success, no device is needed; the Fr result is zero, the support is {0, 0, 0}.  A vector pointer may be NULL iff n == 0.
 *  - Operands are never written; `a` may equal `b` (a sum of squares).
 *  - Refused with hipErrorInvalidValue before anything is launched (and before a device is needed): an unknown op, a NULL result, a NULL `a`
 *    (or, for DOT, `b`) with n > 0; device operands on different devices.
 *  - Workspace (one partial per workgroup, at most 2048 per vector) comes from the calling lane; a repeated call grows nothing
 *    (snarkvm_hip_alloc_stats).
 * The strided forms are batches over device memory like the ones below: member y reads `a` (and `b`, `v`) advanced by y * stride elements,
 * stride >= n, one launch sequence for all; results = count x 32 bytes, out = count x 3 uint64_t, member after member.  b_shared != 0: every
 * member is multiplied by the SAME `b` (the three evaluate_with_coeffs of one matrix, snark/varuna/ahp/matrices.rs:117); otherwise `b`
 * advances like `a`.  count == 0: success, nothing happens. */
enum { SNARKVM_HIP_FR_REDUCE_SUM = 0, SNARKVM_HIP_FR_REDUCE_DOT = 1 };
RustError snarkvm_hip_fr_reduce(int op, void *result, const void *a, const void *b, size_t n, int on_device);
RustError snarkvm_hip_fr_reduce_strided(int op, void *results, const void *a, const void *b, size_t n, size_t count, size_t stride,
                                        int b_shared);
RustError snarkvm_hip_fr_support(uint64_t *out3, const void *v, size_t n, int on_device);
RustError snarkvm_hip_fr_support_strided(uint64_t *out, const void *v, size_t n, size_t count, size_t stride);

/* Evaluation of many polynomials, each at its own point, in one launch sequence (csrc/poly.hip.h: fr_evaluate_kernel, the member of the reduction
 * family that carries the powers of the point; fr_reduce_final_kernel folds the per-workgroup partials): results[k] = sum_{i < lens[k]}
 * polys[k][i] * points[k]^i - DensePolynomial::evaluate (fft/polynomial/dense.rs:98-114), the `evaluations` of a proof (snark/varuna/varuna.rs:583-592)
 * and, by linearity, every value of a linear combination (get_lc_eval, ahp/ahp.rs:469-487): each coefficient is read once, coalesced, five products
 * and one Montgomery reduction per four coefficients.  0^0 = 1 (a zero point yields polys[k][0]); the zero polynomial and a length of 0 yield 0;
 * trailing zero coefficients change nothing.
 *  - polys, lens and points (count x 32 bytes, Montgomery form, ONE point per member) are HOST arrays, read during the call and not retained;
 *    results is count x 32 bytes of HOST memory; on_device governs every polys[k].  Members may overlap and repeat and are never written.  Equal
 *    points are recognised by their bytes and share their powers; a call carries any number of distinct points and any number of members up to
 *    65535 (one kernel launch holds 64 members at 3 distinct points: the call splits itself, and the results depend on no split).
 *  - count == 0: success, nothing is touched.  Every lens[k] == 0: results are zero-filled, no device is needed.  A member pointer may be NULL
 *    iff its length is 0.
 *  - With host operands (on_device = 0) the distinct member buffers are staged into one lane buffer, each uploaded once, and the values are there on
 *    return.  With device operands inside a snarkvm_hip_scope the call is only enqueued on the scope's stream, in order, and the values are
 *    delivered when the scope is flushed (snarkvm_hip_scope_end), like the result of snarkvm_hip_fr_reduce.
 *  - Refused with hipErrorInvalidValue before anything is launched (and, but for the last, before a device is needed), `results` untouched: a NULL
 *    results, polys, lens or points with count > 0; a NULL member of non-zero length; a length above 2^29; count > 65535; with on_device = 1,
 *    members on different devices.
 *  - Workspace (one partial per workgroup and member, at most 2048 per member, the results, and the table of powers of one launch: 72 KB per
 *    point, filled by a launch of its own in front of every evaluation launch) comes from the calling lane; the powers z^(2^i) the table is built
 *    from travel as kernel arguments.  A repeated call grows nothing (snarkvm_hip_alloc_stats). */
RustError snarkvm_hip_fr_evaluate(void *results, size_t count, const void *const *polys, const size_t *lens, const void *points, int on_device);

/* Sparse matrix times vector over a REGISTERED matrix (csrc/poly.hip.h: fr_spmv_seg_kernel, fr_spmv_fix_kernel): the one product of the Varuna
 * prover that is not dense - z_M = M z for M in {A, B, C} (snark/varuna/ahp/prover/round_functions/mod.rs:131-188) and M(alpha, .) = M^T l_alpha
 * (third.rs:303-306, with l_alpha left in device memory by snarkvm_hip_fr_lagrange_coefficients and the result going on to snarkvm_hip_ntt_device).
 * The matrices are circuit data, fixed for the life of a proving key like the SRS: register once, multiply many times.
 * fr_matrix_register: CSR - row r owns entries row_ptr[r] .. row_ptr[r+1]-1 (row_ptr: rows + 1 values); entry k is vals[k] (32 bytes, Montgomery
 * form) at column col_idx[k].  Host arrays, not retained.  Duplicate columns inside a row, rows of any length (empty ones too), rows == 0 and no
 * entries at all are legal; values are not checked to be < r (they are treated like every other Fr operand).  At registration every row is cut
 * into segments of at most S entries and the segment table is uploaded with the entries; one replica per device of the current device set, like
 * registered bases.
 *  - Refused with hipErrorInvalidValue BEFORE a device is needed and before anything is allocated (*handle, when given, is NULL afterwards): a NULL
 *    handle; a NULL row_ptr, or NULL col_idx / vals of a matrix with entries; row_ptr[0] != 0; a decreasing row_ptr; row_ptr[rows] > 2^32 - 1;
 *    rows or cols > 2^28; any col_idx[k] >= cols.  So no index the kernels ever see points outside x.
 * fr_matrix_free: NULL is a no-op.  The replicas are released with hipFree, which returns only when every stream of their device is idle - what
 * snarkvm_hip_free does for device blocks: freeing a handle while a scope of the calling thread still has a product enqueued is safe (the call
 * waits for that product; its result is delivered as usual).
 * fr_spmv: y[r] = sum_k vals[k] * x[col_idx[k]] over row r for r < rows, y[r] = 0 for rows <= r < n_out - ALL n_out elements of every member are
 * written (empty rows give zero), so that z_M lands in a domain-sized buffer that goes straight into snarkvm_hip_ntt_device.  Member m of a batch
 * of `count` reads x + m * stride_x and writes y + m * stride_y (elements); stride_x == 0: every member reads the one x.  count == 1: the strides
 * are ignored.
 *  - on_device = 1: x and y are device pointers on one device; inside a snarkvm_hip_scope the call is only enqueued.  on_device = 0: host
 *    operands, staged like the other passes, the result is there on return.  x is never written.
 *  - Refused with hipErrorInvalidValue, y untouched: a NULL handle; n_out < rows; n_out > 2^28; count > 65535; count > 1 with
 *    0 < stride_x < cols or stride_y < n_out, or a stride of more than 2^40 elements; a NULL y, or a NULL x of a matrix with entries; with on_device = 1 a y that overlaps x (rows are
 *    owned by different waves: an in-place product races) and operands on different devices.
 *  - count == 0, or n_out == 0 for a matrix without rows: success, nothing is touched, no device is needed (n_out == 0 for a matrix WITH rows is
 *    n_out < rows and refused like it).
 *  - No atomics, a fixed order of additions; since field addition is exact and results canonical the 32 bytes of y[r] depend on neither the
 *    segment size, the lane-group width nor the grid.
 *  - Workspace (one partial sum per segment of every row with more than one, per member) comes from the calling lane; a repeated call grows
 *    nothing (snarkvm_hip_alloc_stats). */
typedef struct snarkvm_hip_fr_matrix snarkvm_hip_fr_matrix_t;
RustError snarkvm_hip_fr_matrix_register(snarkvm_hip_fr_matrix_t **handle, size_t rows, size_t cols, const uint64_t *row_ptr, const uint32_t *col_idx,
                                         const void *vals);
void snarkvm_hip_fr_matrix_free(snarkvm_hip_fr_matrix_t *handle);
RustError snarkvm_hip_fr_spmv(void *y, size_t n_out, const snarkvm_hip_fr_matrix_t *handle, const void *x, size_t count, size_t stride_x, size_t stride_y,
                              int on_device);

/* Varuna round 4 over a REGISTERED arithmetization (csrc/poly.hip.h: fr_sumcheck_evals_kernel): the evaluations on K that
 * calculate_matrix_sumcheck_witness (snark/varuna/ahp/prover/round_functions/fourth.rs:155-245) builds per matrix M in {A, B, C} from the circuit's
 * row, col and row_col_val on K (ahp/matrices.rs:101-195) and the challenges alpha, beta.  With r, c, v the three at kappa and
 * d = (alpha - r)(beta - c) (the reference forms it twice: as this product for f, expanded as alpha beta - beta r - alpha c + r c for b):
 *     a[kappa] = a_scale * v        b[kappa] = b_scale * d        f[kappa] = f_scale * v / d, and 0 where d = 0
 * (the zero rule of batch_inversion_and_mul, fields/src/lib.rs:66-129, followed by the product with v).  The caller passes the reference's
 * a_scale = v_R(alpha) v_C(beta), b_scale = |R| |C|, f_scale = a_scale / (|R| |C|).  One fused pass - Montgomery's trick with one shared inversion per
 * thread - where the existing entry points need a dozen launches per matrix.  The arithmetization is circuit data, fixed for the life of a proving
 * key like the SRS and the R1CS matrices: register once, evaluate for every proof.
 * fr_arith_register: row, col, row_col_val are HOST arrays of k elements (32 bytes, Montgomery form), not retained; k need not be a power of
 * two; k == 0 is legal.  One replica per device of the current device set, like snarkvm_hip_fr_matrix_register.
 *  - Refused with hipErrorInvalidValue BEFORE a device is needed and before anything is allocated (*handle, when given, is NULL afterwards): a NULL
 *    handle; a NULL array with k > 0; k > 2^28.
 * fr_arith_free: NULL is a no-op.  The replicas are released with hipFree, which returns only when every stream of their device is idle: freeing a
 * handle while a scope of the calling thread still has an evaluation enqueued is safe, as for snarkvm_hip_fr_matrix_free.
 * fr_matrix_sumcheck_evals: `count` members in ONE launch; member m writes k_m elements (the k of ariths[m]) to each of a_evals[m], b_evals[m],
 * f_evals[m].  alpha, beta and the three scales (a_scale, b_scale, f_scale: 3 x 32 bytes) are HOST values shared by all members - they belong to one
 * circuit (fourth.rs:94-121).  An output pointer, or a whole pointer array, may be NULL: that output is skipped (a call without any f skips the
 * inversion too).
 *  - on_device = 1: the outputs are device pointers on one device; inside a snarkvm_hip_scope the call is only enqueued.  on_device = 0: host
 *    outputs, staged like the other passes, the results are there on return.
 *  - Refused with hipErrorInvalidValue before anything is launched, every output untouched: count > 16; a NULL `ariths` with count > 0 or a NULL
 *    handle in it; NULL alpha, beta or scales; outputs of one call that overlap each other; with on_device = 1 outputs on different devices;
 *    a handle without a replica on the outputs' device.
 *  - count == 0, or every k_m == 0: success, nothing is touched, no device is needed (the same when every output of every member is NULL).
 *  - Workspace: none with on_device = 1 - the running products of the trick are parked in the f output itself before f overwrites them; with
 *    on_device = 0 the staged outputs live in one buffer of the calling lane.  A repeated call grows nothing (snarkvm_hip_alloc_stats).
 *  - No atomics; every thread owns its elements, field arithmetic is exact and results canonical: the 32 bytes of every output depend on neither
 *    the thread count nor the grid. */
typedef struct snarkvm_hip_fr_arith snarkvm_hip_fr_arith_t;
RustError snarkvm_hip_fr_arith_register(snarkvm_hip_fr_arith_t **handle, size_t k, const void *row, const void *col, const void *row_col_val);
void snarkvm_hip_fr_arith_free(snarkvm_hip_fr_arith_t *handle);
RustError snarkvm_hip_fr_matrix_sumcheck_evals(const snarkvm_hip_fr_arith_t *const *ariths, size_t count, void *const *a_evals, void *const *b_evals,
                                               void *const *f_evals, const void *alpha, const void *beta, const void *scales, int on_device);

/* The circuit index: the arithmetization of one R1CS matrix on its non-zero domain K (csrc/poly.hip.h: fr_arithmetize_kernel) - matrix_evals of
 * snark/varuna/ahp/matrices.rs:138-195, the data snarkvm_hip_fr_arith_register takes as three finished host arrays.  The matrix is CSR as in
 * snarkvm_hip_fr_matrix_register: row r owns entries row_ptr[r] .. row_ptr[r+1]-1 (row_ptr: rows + 1 values), entry e is vals[e] (32 bytes, Montgomery
 * form) at column col_idx[e]; nnz = row_ptr[rows].  With w_R, w_C the group generators of the constraint domain (2^lg_constraint elements) and the
 * variable domain (2^lg_variable), for entry e = (val, j) of row i:
 *    row[e] = w_R^i      col[e] = w_C^reindex(j)      row_col[e] = row[e] col[e]      row_col_val[e] = val row_col[e]
 * and (1, 1, 1, 0) at the places nnz <= e < k.  reindex is EvaluationDomain::reindex_by_subdomain (fft/domain.rs:322-344) for the input domain of
 * 2^lg_input elements: with period = 2^(lg_variable - lg_input), j period for j < 2^lg_input, otherwise t + t / (period - 1) + 1 with
 * t = j - 2^lg_input.  k need not be a power of two.  Zero values and duplicate columns are legal (into_matrix_helper's rules are the caller's).
 * fr_arithmetize: each of the four outputs (k elements) may be NULL, which skips it; of a given output every element is written.  on_device governs
 * the CSR arrays AND the outputs: all host memory (0: staged like the other passes, the results are there on return) or all device memory on one
 * device (1; inside a snarkvm_hip_scope the call is only enqueued).  No operand is written.
 *  - k == 0, or all four outputs NULL: success (after the checks below), nothing is touched, no device is needed.
 *  - Refused with hipErrorInvalidValue before anything is launched and before a device is needed, every output untouched: a NULL row_ptr; any lg above
 *    28; lg_input >= lg_variable (the reference's "other.size() must be smaller than self.size()"); k > 2^28; rows > 2^lg_constraint; outputs that
 *    overlap each other or vals; with on_device = 1, operands on different devices or not in device memory.  With HOST CSR arrays (on_device = 0, and
 *    always for fr_arith_register_csr) also: row_ptr[0] != 0; a decreasing row_ptr; row_ptr[rows] > 2^32 - 1; NULL col_idx or vals of a matrix with
 *    entries; k < nnz; any col_idx[e] >= 2^lg_variable.
 *  - With DEVICE CSR arrays their contents cannot be read before the launch and are the CALLER'S CONTRACT, like the registered indices of
 *    snarkvm_hip_fr_spmv: row_ptr[0] = 0, row_ptr non-decreasing, nnz <= k, col_idx[e] < 2^lg_variable; and since nnz is not known before the
 *    launch, of the overlap with vals only its first element is checked - no output may touch the rest either.  The kernel clamps nothing, but it reads nnz
 *    from row_ptr[rows], treats min(nnz, k) places as entries, keeps its row search inside row_ptr whatever that holds and reduces every exponent
 *    modulo its domain size: broken contents give wrong elements, never an access outside row_ptr, col_idx, vals or the outputs.
 * fr_arith_register_csr: HOST CSR arrays, not retained; every device of the current device set computes ITS OWN replica (row | col | row_col_val)
 * with the same kernel - nothing but the CSR arrays crosses the bus.  The handle is indistinguishable from snarkvm_hip_fr_arith_register's: it goes to
 * snarkvm_hip_fr_matrix_sumcheck_evals and is released by snarkvm_hip_fr_arith_free.  Refused like fr_arithmetize with host arrays, and for a NULL
 * handle; *handle, when given, is NULL afterwards.  k == 0 is legal.
 *  - The row of an entry is found by an upper-bound binary search over row_ptr (empty rows - leading, trailing, runs of them - are skipped: the
 *    smallest row whose end lies behind the entry owns it).  A power w^x is the product of two table entries, x's low s bits and the rest
 *    (s = ceil(lg / 2): at most 2 x 2^14 elements per domain).
 *  - Workspace: the two table pairs (built on the device, on the call's stream) and, with host operands, the staged arrays come from the calling lane
 *    and are kept for the next call; a repeated call grows nothing (snarkvm_hip_alloc_stats).
 *  - No atomics; every thread owns its elements, field arithmetic is exact and results canonical: the 32 bytes of every output depend on neither the
 *    table split, the thread count nor the grid. */
RustError snarkvm_hip_fr_arithmetize(void *row, void *col, void *row_col, void *row_col_val, size_t k, size_t rows, const uint64_t *row_ptr,
                                     const uint32_t *col_idx, const void *vals, uint32_t lg_constraint, uint32_t lg_variable, uint32_t lg_input,
                                     int on_device);
RustError snarkvm_hip_fr_arith_register_csr(snarkvm_hip_fr_arith_t **handle, size_t k, size_t rows, const uint64_t *row_ptr, const uint32_t *col_idx,
                                            const void *vals, uint32_t lg_constraint, uint32_t lg_variable, uint32_t lg_input);

/* Strided batches of the passes above on device memory - the same pass over one vector of every proof of a batch proved in lock
 * step (VarunaSNARK::prove_batch, snark/varuna/varuna.rs:336): member y of the batch uses every vector pointer advanced by
 * y * stride elements (stride >= the vector length); ONE kernel launch sequence for the whole batch.  fr_vec_op_strided: `scalar`
 * is shared.  fr_divide_by_linear_strided: one opening `point` for all members (a batch opening at one challenge point,
 * sonic_pc/mod.rs:316-337), `remainders` = count x 32 bytes of HOST memory.  Inside a snarkvm_hip_scope the calls are only
 * enqueued, like their single-vector forms. */
RustError snarkvm_hip_fr_vec_op_strided(int op, void *out, const void *a, const void *b, const void *c, const void *scalar,
                                        size_t n, size_t count, size_t stride);
RustError snarkvm_hip_fr_divide_by_linear_strided(void *quotients, void *remainders, const void *polys, size_t n,
                                                  const void *point, size_t count, size_t stride);
RustError snarkvm_hip_fr_divide_by_vanishing_strided(void *quotients, void *remainders, const void *polys, size_t len,
                                                     size_t domain_size, size_t count, size_t stride);

/* Synthetic base set for benchmarks: out[i] = (start + i) * G as Rust G1Affine (104 B stride) in
 * device memory. */
RustError snarkvm_hip_g1_generate_bases_device(void *d_out, uint64_t start, size_t npoints);

/* Per-phase timing of the most recent profiled MSM / NTT call (synchronous single-lane calls), measured with HIP events on
 * the stream the kernels were launched on.  Enable first; then read `count` (name, milliseconds) pairs. */
void snarkvm_hip_set_profiling(int enabled);
int snarkvm_hip_get_phase_count(void);
const char *snarkvm_hip_get_phase_name(int i);
double snarkvm_hip_get_phase_ms(int i);

/* How the in-library coalescer grouped concurrent callers of proof-sized G1 MSMs so far: out[4] = {batches dispatched, tickets
 * (MSM instances) in them, largest batch, batches of a single ticket}; reset != 0 clears the counters. */
void snarkvm_hip_coalescer_stats(uint64_t *out, int reset);

/* Workspace growth of the library since the last reset: out[5] = {device allocations, device bytes, pinned-host allocations,
 * pinned bytes, microseconds spent inside them}.  Every lane grows its buffers on demand (hipFree / hipMalloc: the one thing here that
 * synchronises the whole device behind the caller's back); a caller that wants an allocation-free timed region warms the same call
 * shape first and can check with this that nothing grew. */
void snarkvm_hip_alloc_stats(uint64_t *out, int reset);

/* Block until all queued work of every device in use has finished. */
RustError snarkvm_hip_synchronize(void);

/* ---------------------------------------------------------------------------------------------
 * Part 3 - test hooks
 * ------------------------------------------------------------------------------------------- */

/* The device arithmetic (ff.hip.h / ec.hip.h) compiled for the host and run on the CPU, so that the
 * limb arithmetic can be checked without a GPU.  field: 0 = Fr, 1 = Fq.  op: 0 add, 1 sub, 2 mul,
 * 3 sqr, 4 inverse, 5 neg, 6 from_bigint, 7 to_bigint, 8 the NTT's lazy chain ((a + b) - b + 2r) * b (Fr; Fq: a * b),
 * 9 diff_of_products(a, b, b, a + b) = a*b - b*(a + b).  Operands / results are in the reference's
 * memory form (Montgomery R = 2^256 / 2^384), n elements of 32 / 48 bytes. */
int snarkvm_hip_selftest_field(int field, int op, const void *a, const void *b, void *out, size_t n);
/* op: 0 = out(Jacobian 144 B) = sum_i (xyzz) points[i] * small_scalars[i] via mixed adds and doublings;
 * exercises every exceptional branch of ec.hip.h on the host. */
int snarkvm_hip_selftest_g1_msm_naive(const void *points_with_infinity, size_t npoints, size_t ffi_affine_sz,
                                      const void *scalars, void *out);
/* The MSM planner (window width, windows, digit rows, buckets, segment length) evaluated on the host:
 * out[10] = {c, W, J, digit rows, buckets per window, total buckets, S, S2, L, wide}.  Returns 0 if consistent. */
int snarkvm_hip_selftest_msm_plan(size_t n, int window_bits, int tables, int table_bits, uint32_t *out);
/* The host-side finish of an MSM on its own (no device): out (144 B) = sum_i 2^pos[i] * planes[i] over n G1Projective
 * memory images - the Horner chain that combines the bit-plane sums the device leaves (and the per-device partial results of
 * a split MSM, the reference's host `dadd`, snarkvm.cu:290-295).  Returns 0. */
int snarkvm_hip_selftest_g1_finish(const void *planes_projective, const int32_t *pos, size_t n, void *out);
/* The lazily reduced arithmetic of the accumulate kernel (csrc/ffl.hip.h) against the exact arithmetic, on the host: `iters`
 * chained mixed additions (doublings, cancellations and restarts from infinity included) compared coordinate by coordinate,
 * then the field routines at the edges of their operand ranges.  0 = identical; > 0: first differing step; < 0: field case. */
int snarkvm_hip_selftest_fq_lazy(uint64_t seed, int iters);
/* host only: the tail arithmetic of a G1 MSM (ffl.hip.h::fqz_t under the generic addition / doubling laws) against the exact one */
int snarkvm_hip_selftest_g1_lazy_tail(uint64_t seed, int iters);
/* The lane-pair Fq2 arithmetic of the G2 accumulate kernel (csrc/ffl2p.hip.h: the c0 component of every value on the even lane, c1 on
 * the odd lane, operands exchanged inside the VALU) with both lanes of a pair run side by side on the host - the same source - against
 * the exact arithmetic: `iters` chained mixed additions of +- points[k] (npoints >= 2 Rust G2Affine records on the curve, 200-byte stride), restarts
 * from infinity included, every coordinate compared after every step; doublings and cancellations are resolved inside the pair arithmetic.
 * 0 = identical; > 0: first differing step; < 0: a conversion case. */
int snarkvm_hip_selftest_fq2_pair(const void *points, size_t npoints, uint64_t seed, int iters);
/* The sixteen-lane cooperative Fq2 addition of the G2 tail trees (csrc/hex2.hip.h: lane 4 q + p of a DPP row computes Fq sub-product p of the quad
 * schedule's product q; pair exchange, combine, gather) run over sixteen simulated lanes on the host - the same source - against the exact addition:
 * `iters` additions of partial sums of +- points[k], with operands at infinity, P + P and P - P among them.  0 = every lane of every addition ends
 * with exactly the exact sum; > 0: first differing iteration. */
int snarkvm_hip_selftest_g2_hex(const void *points, size_t npoints, uint64_t seed, int iters);
/* Device check: the G2 fold / bit-plane kernels launched `iters` times over one fixed set of partial-sum lists (2^(m + hb) buckets) must leave
 * the same group elements.  report[10]: [0] fold launches differing from the first, [1] differing fold slots, [2] bit-plane launches differing,
 * [3] differing planes, [4..7] first differing fold slots, [8], [9] fold slots / planes the fast kernels handed to the fix kernels (equal x met). */
RustError snarkvm_hip_devtest_g2_tail_repeat(const void *points, size_t npoints, int m, int hb, int threads, int plane_threads,
                                             int hex, int quads, int iters, uint32_t *report);
/* The NTT's planner, power tables and index maps (csrc/ntt.hip.h) run on the host through the kernels' own __host__ __device__ code.
 * ntt_plan: out[4] = the pass radices (log2) of the 2^lg plan; returns the number of passes, -1 when lg > 28. */
int snarkvm_hip_selftest_ntt_plan(uint32_t lg, int32_t *out);
/* kind 0: out[i] = the closing twiddle pass `pass` of the 2^lg transform multiplies by for inner * k = x[i] (pass = -1: W^x[i] with W the
 * primitive 2^28-th root); kind 1: out[i] = g^x[i], g = 22.  inverse = 1: of W^-1 / g^-1.  n values of 32 bytes, memory Montgomery form.
 * 0, or -1 when an argument or exponent is out of range. */
int snarkvm_hip_selftest_ntt_twiddle(int kind, uint32_t lg, int pass, int inverse, const uint64_t *x, size_t n, void *out);
/* The tile addressing of every pass and the last pass' output index map of the 2^lg plan (plan = NULL: the backend's; else npass forced
 * radices), indices only: returns the number of positions read or written twice, or holding another coefficient than NN order puts there. */
int snarkvm_hip_selftest_ntt_index(uint32_t lg, const int32_t *plan, int npass);
/* The whole NN transform of 2^lg <= 2^16 elements (memory form, in place) computed on the host pass by pass in exact arithmetic over the
 * kernels' addressing, twiddles, coset powers and output map (plan = NULL: the backend's plan; else npass forced radices).  0, or -1. */
int snarkvm_hip_selftest_ntt_host(void *inout, uint32_t lg, const int32_t *plan, int npass, int dir, int type);
/* snarkvm_hip_fr_lincomb over host memory with the CPU in the kernel's place: the same validation, operand order and split into launches,
 * every launch a loop over i through the kernel's own per-element routine (csrc/poly.hip.h: fr_lincomb_at, Fp::sum_of_products).  0, or -1
 * when the arguments are refused. */
int snarkvm_hip_selftest_fr_lincomb(void *out, size_t n_out, size_t count, const void *const *polys, const size_t *lens, const void *coeffs);
/* snarkvm_hip_fr_open_fold over host memory with the CPU in the kernels' place, over a GIVEN geometry: the same validation, operand order and
 * split into launches, every launch a loop over its threads through the kernels' own per-thread routines (csrc/poly.hip.h: fr_lincomb_at,
 * fr_open_up_chunk, fr_open_down_chunk, the scan step and carry routines), a workgroup's exchanges through LDS as loops over its threads.
 *   route 1 (a quotient is required): the scan form - workgroups of 256 threads, C >= 1 coefficients per thread, `blocks` workgroups with
 *           ceil(n / (256 C)) <= blocks <= 257 (a workgroup past the end owns nothing)
 *   route 0: the chunk recursion - chunks of C >= 2 coefficients at every level, blocks = ceil(ceil(n / C) / 256), the workgroups of level 0
 * 0, or -1 when the arguments or the geometry are refused.  fr_open_fold_geometry: out5 = {route, C, blocks} of what the device call launches
 * for n coefficients when a quotient is wanted (without one: always route 0, C = 32), the operands per table (FR_LINCOMB_CHUNK) and the
 * terms the fused sweep takes at most (FR_OPEN_FUSE). */
int snarkvm_hip_selftest_fr_open_fold(void *quotient, void *remainder, size_t n, size_t count, const void *const *polys, const size_t *lens,
                                      const void *coeffs, const void *point, int route, uint32_t C, uint32_t blocks);
int snarkvm_hip_selftest_fr_open_fold_geometry(size_t n, uint32_t *out5);
/* snarkvm_hip_fr_selector_fold over host memory with the CPU in the kernels' place: the same validation, member tables and split into launches,
 * every launch a loop over i through the kernel's own per-index routine (csrc/poly.hip.h: fr_selector_at), then the tiling of xg_out.  0, or
 * -1 when the arguments are refused. */
int snarkvm_hip_selftest_fr_selector_fold(void *h_out, size_t h_len, void *xg_out, size_t target_size, void *sums, size_t count,
                                          const void *const *polys, const size_t *lens, const size_t *src_sizes, const void *multipliers);
/* snarkvm_hip_fr_witness_evals over host memory with the CPU in the kernel's place: the same validation, then a loop over k through the kernel's
 * own per-index routine (csrc/poly.hip.h: fr_witness_at).  0, or -1 when the arguments are refused. */
int snarkvm_hip_selftest_fr_witness_evals(void *out, size_t n, const void *w, size_t w_len, const void *x_evals, size_t input_size);
/* snarkvm_hip_fr_assignment_evals over host memory with the CPU in the kernel's place, over a GIVEN thread count (`threads` >= 1 per member, thread
 * t owning k = t, t + threads, ...): the same validation, every element through the kernel's own per-index routine (csrc/poly.hip.h:
 * fr_assignment_at).  0, or -1 when the arguments are refused.  fr_assignment_geometry: out3 = {workgroups, threads per workgroup} the device call
 * launches per member of n elements, and the cap on the workgroups; 0, or -1 for a NULL out3 or n > 2^28. */
int snarkvm_hip_selftest_fr_assignment_evals(void *out, size_t n, const void *vars, size_t num_vars, size_t input_size, size_t count,
                                             size_t stride_out, size_t stride_vars, uint32_t threads);
int snarkvm_hip_selftest_fr_assignment_geometry(size_t n, uint32_t *out3);
/* snarkvm_hip_fr_rowcheck_fold over host memory with the CPU in the kernel's place: the same validation, member tables and split into launches,
 * every launch a loop over i through the kernel's own per-index routine (csrc/poly.hip.h: fr_rowcheck_at), the violation bits it returns counted
 * per member.  0, or -1 when the arguments are refused. */
int snarkvm_hip_selftest_fr_rowcheck_fold(void *out, uint64_t *violations, size_t n, size_t count, const void *const *a, const void *const *b,
                                          const void *const *c, const void *multipliers);
/* what snarkvm_hip_fr_rowcheck_fold was built with: out2 = {members per launch (FR_ROWCHECK_CHUNK), members per Montgomery reduction} */
int snarkvm_hip_selftest_fr_rowcheck_geometry(uint32_t *out2);
/* snarkvm_hip_fr_reduce / snarkvm_hip_fr_support over host memory with the CPU in the kernels' place, over a GIVEN launch geometry (blocks >= 1
 * workgroups of threads = 64, 128 or 256): every thread's private accumulation and every combine step through the kernels' own routines
 * (csrc/poly.hip.h: fr_reduce_thread, fr_support_thread, fr_support_combine), the trees level by level over the lanes they exchange between, the
 * second launch included.  0, or -1 when the arguments are refused.  fr_reduce_geometry: out4 = {workgroups, threads per workgroup} the device
 * call launches for n elements, the cap on the workgroups, and the number of products per Montgomery reduction of the inner product. */
int snarkvm_hip_selftest_fr_reduce(int op, void *out, const void *a, const void *b, size_t n, uint32_t blocks, uint32_t threads);
int snarkvm_hip_selftest_fr_support(uint64_t *out3, const void *v, size_t n, uint32_t blocks, uint32_t threads);
int snarkvm_hip_selftest_fr_reduce_geometry(size_t n, uint32_t *out4);
/* snarkvm_hip_fr_evaluate over host memory with the CPU in the kernels' place, over a GIVEN launch geometry (blocks >= 1 workgroups of threads = 64,
 * 128 or 256 per member, blocks x threads <= 2^19): the same validation, the same grouping of the points and split into launches, every thread's
 * Horner walk and power of the point, thread 0's factor on the workgroup's sum, the table of powers both come from and every combine step through
 * the kernels' own routines (csrc/poly.hip.h: fr_evaluate_table_entry, fr_evaluate_thread, fr_evaluate_block, fr_reduce_thread), the trees level by
 * level, the last launch included.  0, or -1 when the
 * arguments are refused or the kernel does not take the geometry.  fr_evaluate_geometry: out (8 values) = {workgroups per member, threads per
 * workgroup} the device call launches for a longest member of n_max, the cap on the workgroups, the coefficients per Montgomery reduction, the
 * members and the distinct points one launch holds, how the power of the thread index is formed (2: one factor per thread and one per workgroup,
 * both from a table in lane workspace; 0: the same two factors from the set bits of the exponent, in place; 1: per thread alone, in place) and the
 * bits of a thread index the powers z^(2^i) cover. */
int snarkvm_hip_selftest_fr_evaluate(void *results, size_t count, const void *const *polys, const size_t *lens, const void *points, uint32_t blocks,
                                     uint32_t threads);
int snarkvm_hip_selftest_fr_evaluate_geometry(size_t n_max, uint32_t *out);
/* snarkvm_hip_fr_spmv (count = 1) over host memory with the CPU in the kernels' place, for a GIVEN segment size `seg` >= 1 and lane-group width
 * (4, 8, 16 or 64): the validation and the segmentation of snarkvm_hip_fr_matrix_register, every lane through the kernels' own accumulate routine
 * (csrc/poly.hip.h: fr_spmv_lane over Fp::sum_of_products), the butterfly level by level, the partials and the fix-up launch in the same order.  0, or
 * -1 when the arguments are refused.  fr_spmv_geometry: out4 = {segment size S, lane-group width, threads per workgroup, segments} of what
 * registration lays out for a matrix of `rows` rows whose nnz entries are spread evenly (the first nnz % rows rows hold one more). */
int snarkvm_hip_selftest_fr_spmv(void *y, size_t n_out, size_t rows, size_t cols, const uint64_t *row_ptr, const uint32_t *col_idx, const void *vals,
                                 const void *x, uint32_t seg, uint32_t width);
int snarkvm_hip_selftest_fr_spmv_geometry(size_t rows, size_t nnz, uint32_t *out4);
/* snarkvm_hip_fr_matrix_sumcheck_evals for one member over host memory with the CPU in the kernel's place, over a GIVEN geometry: blocks x threads
 * threads in all (any counts >= 1; more threads than elements is allowed), thread t owning t, t + T, ... through the kernel's own per-thread routine
 * and the same host-side constants (csrc/poly.hip.h: fr_sumcheck_thread, fr_sumcheck_consts).  a, b, f may be NULL (skipped).  0, or -1 when the
 * arguments are refused.  fr_sumcheck_geometry: out4 = {threads T, threads per workgroup, workgroups, elements per thread (the share the thread
 * count is derived from)} of what the device call launches for a member of k elements; 0, or -1 for a NULL out or k > 2^28. */
int snarkvm_hip_selftest_fr_sumcheck(void *a, void *b, void *f, const void *row, const void *col, const void *rcv, size_t k, const void *alpha,
                                     const void *beta, const void *scales, uint32_t blocks, uint32_t threads);
int snarkvm_hip_selftest_fr_sumcheck_geometry(size_t k, uint32_t *out);
/* snarkvm_hip_fr_arithmetize over host memory with the CPU in the kernels' place, for a GIVEN table split (the low split_bits bits of an exponent go
 * to the first table; a value above a domain's lg counts as that lg) and `threads` >= 1 threads in all, thread t owning e = t, t + threads, ...: the
 * validation of the host-operand call, the tables and every element through the kernels' own routines (csrc/poly.hip.h: fr_arith_table_at,
 * fr_arith_at).  0, or -1 when the arguments are refused.  fr_arithmetize_geometry: out4 = {workgroups, threads per workgroup, the cap on the
 * workgroups} of what the device call launches for k elements, and the split bits it uses for a domain of 2^lg elements. */
int snarkvm_hip_selftest_fr_arithmetize(void *row, void *col, void *row_col, void *row_col_val, size_t k, size_t rows, const uint64_t *row_ptr,
                                        const uint32_t *col_idx, const void *vals, uint32_t lg_constraint, uint32_t lg_variable, uint32_t lg_input,
                                        uint32_t split_bits, uint32_t threads);
int snarkvm_hip_selftest_fr_arithmetize_geometry(size_t k, uint32_t lg, uint32_t *out4);
/* Same field operations executed by a GPU kernel (one thread per element). */
RustError snarkvm_hip_devtest_field(int field, int op, const void *a, const void *b, void *out, size_t n);
/* Field arithmetic that the two operands of snarkvm_hip_selftest_field cannot express, one case per record, operands and results in memory
 * form.  op (input record -> output record, in field elements of 32 B (Fr) / 48 B (Fq), an Fq2 element = c0 then c1):
 *   0  Fq diff_of_products: a, b, c, d -> a*b - c*d          1  the same over Fr
 *   2  Fq2 mul: a, b -> a*b      3  Fq2 sqr: a -> a^2        4  Fq2 inverse: a -> 1/a (a != 0)
 *   5  Fq2 diff_of_products: a, b, c, d -> a*b - c*d
 *   6  Fq sqrt: a -> root (48 B), then ok as four 32-bit words {ok, 0, 0, 0}: ok = 0 and root = 0 for a non-residue
 *   7  Fq2 sqrt: a -> root (96 B), then {ok, 0, 0, 0}: ok = 0 where the reference's Fp2::sqrt returns None
 *   8  Fq raw: a, b -> a + b, a - b, -a, 2a, a * b, 0 * 0 - a * b as the arithmetic's INTERNAL limbs (a 2^377 mod q, 29-bit limbs packed into 48 B)
 *      without the conversion back to memory form, so that a result that is not canonical (q instead of 0) shows      9  the same over Fr (2^261)
 * selftest: on the host (the same source as the kernels, square roots included), returns 0, or 1 for a bad argument; devtest: one GPU thread per case. */
int snarkvm_hip_selftest_field_ext(int op, const void *in, void *out, size_t n);
RustError snarkvm_hip_devtest_field_ext(int op, const void *in, void *out, size_t n);
/* The lazily reduced signed-limb arithmetic of the bucket-accumulation loops (csrc/ffl.hip.h, ffl2.hip.h, ffl2p.hip.h), one case per record.
 * Operands and results are RAW limbs: a value V = 13 int32 words v_0 .. v_12 (value = sum v_i 2^(29 i), signed), a flag = one word; nothing
 * normalises or reduces a result on the way out.  op (input record -> output record, in 32-bit words):
 *   0  fql_t::mul: a, b -> V                 1  fql_t::sqr: a -> V                 2  fql_t::diff_of_products: a, b, c, d -> V
 *   3  normalized: a -> V                    4  to_exact: a -> the 13 limbs of the canonical fq_t (x 2^377)
 *   5  from_exact: 13 limbs of a canonical fq_t -> V                6  store_raw / load_raw: a -> the 12 words of the image, then load_raw of it
 *   7  fqz_t: a, b, z -> a + b, a - b, a.dbl(), a.neg(), then the word z.is_zero()
 *   8  xyzz_lazy_t::madd: x, y, zz, zzz, inf, px, py, negate -> the returned bool, x, y, zz, zzz, inf
 *   9  per-lane helpers of the pair addition: a, b, c, t, y -> p = sub_norm(a, b, 1), sub_norm(a, c, -1), norm_k(t), cond_neg_canonical(y, true),
 *      cond_neg_canonical(y, false), then the word is_zero_mod_q(p)
 *  10  the pair product: a.c0, a.c1, b.c0, b.c1 -> per component (c0, then c1) the product's component, then the lane's prepared operands as the
 *      exchange left them: opa_t X, Y (13 + 13 words), opb_t recv (14 words)
 *  11  fq2p::xyzz_pair_t::madd: x.c0, x.c1, y.c0, y.c1, zz.c0, zz.c1, zzz.c0, zzz.c1, inf, px.c0, px.c1, py.c0, py.c1, negate -> the eight
 *      components, inf
 * selftest: on the host (ops 10, 11 through the two-lane host exchange), returns 0, or 1 for a bad argument; devtest: workgroups of 64 threads, one
 * thread per case for ops 0 - 9, one DPP lane pair per case (even lane c0, odd lane c1) for ops 10, 11; n <= 2^24. */
int snarkvm_hip_selftest_lazy_ext(int op, const void *in, void *out, size_t n);
RustError snarkvm_hip_devtest_lazy_ext(int op, const void *in, void *out, size_t n);
/* The scalar-read phase of a variable-base MSM on its own: n host scalars (32 B each; montgomery = 1: Fr memory images) go through the plan and the
 * digit parameters a device-side MSM of this geometry gets (window_bits, tables, table_bits as a registered handle passes them; a fused batch asks
 * for table_bits-wide windows) and through the stand-alone digit kernel that MSM would launch - u16 digits up to 16-bit windows, u32 digits above;
 * `digits` receives the matrix [digit rows][columns] of raw digits u = ((s + bias) >> c * row) & (2^c - 1), signed digit d = u - 2^(c-1).
 * multi = 1: the digit kernel of a fused batch over two instances, scalars [0, n) and scalars [n / 2, n), laid side by side in the padded
 * concatenation (each starts on a multiple of 8 192 columns; the padding holds the zero digit u = 2^(c-1)).
 * info[6] = {c, digit rows, bytes per digit, columns, first column of the second instance, scalars of the second instance} (the last two 0 unless
 * multi).  digits_bytes must be digit rows * columns * bytes per digit exactly (the planner is snarkvm_hip_selftest_msm_plan), n >= 1. */
RustError snarkvm_hip_devtest_msm_digits(const void *scalars, size_t n, int window_bits, int tables, int table_bits, int montgomery, int multi,
                                         void *digits, size_t digits_bytes, uint32_t *info);
/* The tail kernels of a variable-base MSM (csrc/msm.hip.h 6.-7b), unmodified, launched ONCE over caller-chosen partial-sum lists; every output comes
 * back as an exact projective point (the reference's Projective image: 144 B for G1, 288 B for G2).
 * arith: 0 = G1 on the exact arithmetic, 1 = G1 on the lazy tail arithmetic, 2 = G2 (hipErrorNotSupported in a build without G2).
 * stage: 0 = reduce round, 1 = bucket merge, 2 = fold, fold fix, dense bit planes, plane fix, 3 = the bit planes of unfolded windows.
 * geom[12] = {m, hb, W, nb, S2, L, slot, fold threads, plane threads, hex, quads (bit 0: planes, bit 1: fold), run_fix (G2: launch the fix kernels)};
 * a stage reads its own members only.  Buckets nbt: stage 0, 1: any (<= 2^17); stage 2: W * 2^(m + hb); stage 3: W * nb.
 * points: npoints affine points in the Rust layout (G1 104 B, G2 200 B stride), none at infinity.  Entry e is the exact sum of +- points[|t| - 1] over
 * its terms t = terms[3 e .. 3 e + 2] (0 = none; no term = the point at infinity, an all-zero image), formed with the mixed addition; seeds[e] != 0
 * replaces it by another representative (l^2 X, l^3 Y, l^2 ZZ, l^3 ZZZ), l derived from the seed.  Entries [0, nentries) are the lists' partial sums,
 * bucket k owning entries start[k] .. start[k] + cnt[k] - 1 (start holds nbt + 1 values); stage 1: entries [nentries, nentries + nbt * L) are the
 * initial content of the accumulator.
 * Every output buffer is filled with 0xff bytes before the launch (the accumulator of stage 1 excepted).  out holds nout points, status and flags
 * nout words each: status 0 = written, 1 = the device image is still the fill pattern (the point is then meaningless), 2 = (stage 1) the device
 * image is bit for bit what was put in; flags: the word the fast G2 kernel left for that output (0xffffffff: none written; G1: 0).
 *   stage 0: nout >= the number T of partial sums the round leaves (the grid covers nout, as the launcher's covers its bound); aux[nbt + 1] receives
 *            start_out.           stage 1: nout = nbt * L.
 *   stage 2: nout = W * 2^(m + 1) fold slots, then 2 W (m + 1) planes.      stage 3: nout = W * nbits planes, nbits = log2(nb) + 1.
 * hipErrorInvalidValue: a null pointer, hb > m, hb > 11, nb > 1024 or not a power of two, threads other than 64 / 128 / 256, quads with 64 threads,
 * hex or run_fix outside G2, lists that overrun the entries or are not laid out bucket after bucket where a kernel relies on that, a wrong nout. */
RustError snarkvm_hip_devtest_msm_tail(int arith, int stage, const int32_t *geom, const void *points, size_t npoints, const int32_t *terms,
                                       const uint64_t *seeds, size_t nentries, const uint32_t *start, const uint32_t *cnt, size_t nbt, void *out,
                                       uint32_t *status, uint32_t *flags, size_t nout, uint32_t *aux);

#ifdef __cplusplus
}
#endif
#endif /* SNARKVM_HIP_H */
