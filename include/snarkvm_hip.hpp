// snarkvm_hip.hpp - C++ host mirror of the reference's accelerator crate `snarkvm_algorithms_cuda`
// (algorithms/cuda/src/lib.rs:77-168): the same three functions NTT / polymul / msm with the same argument
// meaning and error behaviour, over the C ABI of snarkvm_hip.h.  Header-only; link with -lsnarkvm_hip.
//
// `Err(cuda::Error)` becomes a thrown snarkvm_hip::Error (code + message); the two argument checks the Rust
// wrapper performs before the FFI call (power-of-two domain, lib.rs:84-86,107-109; npoints <= points.len(),
// lib.rs:150-152) throw std::invalid_argument, mirroring Rust's panic.
#pragma once
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "snarkvm_hip.h"

namespace snarkvm_hip {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
inline void check(RustError e) {
    if (e.code != 0) {
        std::string m = e.message ? e.message : "";
        std::free(e.message);  // the callee allocated it (TAKE_RESPONSIBILITY_FOR_ERROR_MESSAGE, build.rs:79)
        throw Error(e.code, m);
    }
}

// lib.rs:77-97.  Domains up to 2^28; a larger one throws Error with code hipErrorMemoryAllocation (the caller's CPU path).
template <class T>
inline void NTT(size_t domain_size, T* inout, NTTInputOutputOrder order, NTTDirection direction, NTTType type) {
    static_assert(sizeof(T) == 32, "the NTT operates on 32-byte Fr elements (fft/domain.rs:377)");
    if (domain_size == 0 || (domain_size & (domain_size - 1)) != 0) throw std::invalid_argument("domain_size is not power of 2");
    uint32_t lg = 0;
    while (((size_t)1 << lg) < domain_size) lg++;
    check(snarkvm_ntt(inout, lg, order, direction, type));
}

// lib.rs:100-145: returns a vector of `domain` elements pre-filled with `zero`; domains up to 2^28, as for NTT
template <class T>
inline std::vector<T> polymul(size_t domain, const std::vector<std::vector<T>>& polynomials,
                              const std::vector<std::vector<T>>& evaluations, const T& zero) {
    static_assert(sizeof(T) == 32, "Fr elements are 32 bytes");
    if (domain == 0 || (domain & (domain - 1)) != 0) throw std::invalid_argument("domain_size is not power of 2");
    uint32_t lg = 0;
    while (((size_t)1 << lg) < domain) lg++;
    std::vector<const void*> pptrs, eptrs;
    std::vector<size_t> plens, elens;
    for (auto& p : polynomials) {
        pptrs.push_back(p.data());
        plens.push_back(p.size());
    }
    for (auto& e : evaluations) {
        eptrs.push_back(e.data());
        elens.push_back(e.size());
    }
    std::vector<T> out(domain, zero);
    check(snarkvm_polymul(out.data(), pptrs.size(), pptrs.data(), plens.data(), eptrs.size(), eptrs.data(), elens.data(), lg));
    return out;
}

// lib.rs:148-168
template <class Affine, class Projective, class Scalar>
inline Projective msm(const Affine* points, size_t npoints_available, const Scalar* scalars, size_t nscalars) {
    static_assert(sizeof(Scalar) == 32, "scalars are BigInteger256");
    if (nscalars > npoints_available) throw std::invalid_argument("length mismatch: fewer points than scalars");
    Projective ret;
    check(snarkvm_msm(&ret, points, nscalars, scalars, sizeof(Affine)));
    return ret;
}

// Opt-in base cache of msm() (snarkvm_hip.h: snarkvm_hip_set_base_cache*): tables 0 (off), 1, 2, 4, 8 or 16; verified = every byte of
// every hit is compared with a host copy taken at registration.
inline void set_base_cache(int tables, bool verified = false) {
    check(verified ? snarkvm_hip_set_base_cache_verified(tables) : snarkvm_hip_set_base_cache(tables));
}
// {lookups, hits, registrations, verification mismatches, bytes compared, microseconds waited for a comparison, tables, verified}
struct BaseCacheStats {
    uint64_t v[8];
};
inline BaseCacheStats base_cache_stats(bool reset = false) {
    BaseCacheStats s{};
    snarkvm_hip_base_cache_stats(s.v, reset ? 1 : 0);
    return s;
}

// ---- extensions (part 2 of rust/snarkvm-algorithms-hip/src/lib.rs: `resident`) -------------------------------------------
// Deferred-synchronisation scope (snarkvm_hip.h: snarkvm_hip_scope_begin / _end): device-resident calls of this thread between
// construction and destruction are enqueued on one stream and waited for once.  Not copyable; end() reports errors, the
// destructor swallows them (like the Rust guard's Drop).
class Scope {
public:
    // flags: 0, or SNARKVM_HIP_SCOPE_ASYNC_MSM (registered-bases MSMs over device scalars are enqueued too; their outputs are written by end())
    // [| SNARKVM_HIP_SCOPE_STABLE_INPUTS: the scalar vectors of those MSMs are not touched before end()]
    explicit Scope(const void* d_any = nullptr, uint32_t flags = 0) { check(snarkvm_hip_scope_begin_ex(d_any, flags)); }
    void* stream() const { return snarkvm_hip_scope_stream(); }  // the hipStream_t of the scope's calls
    void set_flags(uint32_t flags) { check(snarkvm_hip_scope_set_flags(flags)); }  // for the calls that follow (e.g. | SNARKVM_HIP_SCOPE_MSM_IN_STREAM after the independent MSM is out)
    void collect(const void* out = nullptr) { check(snarkvm_hip_scope_collect(out)); }  // the outputs of that MSM call (null: of all enqueued so far); the scope stays open
    Scope(const Scope&) = delete;
    Scope& operator=(const Scope&) = delete;
    void end() {
        if (open_) {
            open_ = false;
            check(snarkvm_hip_scope_end());
        }
    }
    ~Scope() {
        if (open_) {
            RustError e = snarkvm_hip_scope_end();
            if (e.message) std::free(e.message);
        }
    }

private:
    bool open_ = true;
};

// Device memory owned through the library (snarkvm_hip_malloc / _free / _memcpy_*; rust: resident::DeviceBuffer): the operands of every `d_*`
// argument of the extension ABI without a HIP header on the caller's side.  Host-side copies are complete on return; copy_from() / fill() inside a
// Scope are only enqueued on the scope's stream.  Not copyable; movable.
class DeviceBuffer {
public:
    DeviceBuffer() = default;
    explicit DeviceBuffer(size_t bytes, int device = -1) : bytes_(bytes) { check(snarkvm_hip_malloc(&p_, bytes, device)); }
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    DeviceBuffer(DeviceBuffer&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr, o.bytes_ = 0; }
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
        if (this != &o) {
            release();
            p_ = o.p_, bytes_ = o.bytes_;
            o.p_ = nullptr, o.bytes_ = 0;
        }
        return *this;
    }
    ~DeviceBuffer() { release(); }
    void* data() const { return p_; }
    size_t size() const { return bytes_; }
    void* at(size_t byte_offset) const {
        if (byte_offset > bytes_) throw std::out_of_range("DeviceBuffer::at");
        return static_cast<char*>(p_) + byte_offset;
    }
    void upload(const void* src, size_t bytes, size_t byte_offset = 0) const {
        if (byte_offset + bytes > bytes_) throw std::out_of_range("DeviceBuffer::upload");
        check(snarkvm_hip_memcpy_h2d(at(byte_offset), src, bytes));
    }
    void download(void* dst, size_t bytes, size_t byte_offset = 0) const {
        if (byte_offset + bytes > bytes_) throw std::out_of_range("DeviceBuffer::download");
        check(snarkvm_hip_memcpy_d2h(dst, at(byte_offset), bytes));
    }
    void copy_from(size_t byte_offset, const void* d_src, size_t bytes) const {
        if (byte_offset + bytes > bytes_) throw std::out_of_range("DeviceBuffer::copy_from");
        check(snarkvm_hip_memcpy_d2d(at(byte_offset), d_src, bytes));
    }
    void fill(size_t byte_offset, int value, size_t bytes) const {
        if (byte_offset + bytes > bytes_) throw std::out_of_range("DeviceBuffer::fill");
        check(snarkvm_hip_memset(at(byte_offset), value, bytes));
    }

private:
    void release() {
        if (p_) {
            RustError e = snarkvm_hip_free(p_);
            if (e.message) std::free(e.message);
            p_ = nullptr;
        }
    }
    void* p_ = nullptr;
    size_t bytes_ = 0;
};

// polymul over operands in device memory (snarkvm_hip.h: snarkvm_hip_polymul_device): d_out (2^lg elements, all written) = the product of the
// coefficient-form operands `polys` ({device pointer, length <= 2^lg}) and the evaluation vectors `evals` (2^lg elements each).  No operand is
// written; d_out may be the start of one of them.  Inside a Scope the call is only enqueued.
struct DevicePoly {
    const void* data;
    size_t len;
};
inline void polymul_device(uint32_t lg, void* d_out, const std::vector<DevicePoly>& polys, const std::vector<const void*>& evals = {}) {
    std::vector<const void*> pptrs;
    std::vector<size_t> plens, elens(evals.size(), (size_t)1 << lg);
    for (auto& p : polys) {
        pptrs.push_back(p.data);
        plens.push_back(p.len);
    }
    check(snarkvm_hip_polymul_device(d_out, pptrs.size(), pptrs.data(), plens.data(), evals.size(), evals.data(), elens.data(), lg));
}

// Linear combination of polynomials in one device pass (snarkvm_hip.h: snarkvm_hip_fr_lincomb): out[i] = sum_k coeffs[k] * polys[k][i] for
// i < n_out, polys[k] counting as zero from its length (<= n_out) on.  coeffs: polys.size() x 32 bytes of HOST memory, Montgomery form;
// on_device governs `out` and every polys[k].data.  No operand is written; out may be the start of one of them.  With on_device inside a
// Scope the call is only enqueued; a divide_by_linear over `out` then yields the opening quotient and the combination's evaluation.
inline void fr_lincomb(void* out, size_t n_out, const std::vector<DevicePoly>& polys, const void* coeffs, bool on_device) {
    std::vector<const void*> pptrs;
    std::vector<size_t> plens;
    for (auto& p : polys) {
        pptrs.push_back(p.data);
        plens.push_back(p.len);
    }
    check(snarkvm_hip_fr_lincomb(out, n_out, pptrs.size(), pptrs.data(), plens.data(), coeffs, on_device ? 1 : 0));
}

// Opening fold (snarkvm_hip.h: snarkvm_hip_fr_open_fold): comb = sum_k coeffs[k] * polys[k] over n coefficients, formed once; quotient (n elements,
// all written, or nullptr) = comb / (X - point) with a trailing zero; remainder (32 bytes of HOST memory, or nullptr) = comb(point).  coeffs:
// polys.size() x 32 bytes of HOST memory, Montgomery form; point: 32 bytes of HOST memory; on_device governs `quotient` and every polys[k].data.
// No operand is written and none may overlap the quotient.  With on_device inside a Scope the call is only enqueued and the remainder arrives
// when the Scope ends.
inline void fr_open_fold(void* quotient, void* remainder, size_t n, const std::vector<DevicePoly>& polys, const void* coeffs, const void* point, bool on_device) {
    std::vector<const void*> pptrs;
    std::vector<size_t> plens;
    for (auto& p : polys) {
        pptrs.push_back(p.data);
        plens.push_back(p.len);
    }
    check(snarkvm_hip_fr_open_fold(quotient, remainder, n, pptrs.size(), pptrs.data(), plens.data(), coeffs, point, on_device ? 1 : 0));
}

// The sums of Varuna's round 3 in one device pass (snarkvm_hip.h: snarkvm_hip_fr_selector_fold): member k = members[k] with source domain
// src_sizes[k] and multiplier multipliers[k] (members.size() x 32 bytes of HOST memory, Montgomery form).  h_out (h_len coefficients): the sum of
// the scaled quotients by X^n_k - 1; xg_out (target_size coefficients): the sum of the scaled remainders, tiled; sums (members.size() elements):
// the sum of every unscaled member over its source domain.  Each output may be nullptr (skipped); on_device governs the outputs and every
// members[k].data.  No member is written.  With on_device inside a Scope the call is only enqueued.
inline void fr_selector_fold(void* h_out, size_t h_len, void* xg_out, size_t target_size, void* sums, const std::vector<DevicePoly>& members,
                             const std::vector<size_t>& src_sizes, const void* multipliers, bool on_device) {
    if (src_sizes.size() != members.size()) throw std::invalid_argument("fr_selector_fold: one source domain per member");
    std::vector<const void*> pptrs;
    std::vector<size_t> plens;
    for (auto& p : members) {
        pptrs.push_back(p.data);
        plens.push_back(p.len);
    }
    check(snarkvm_hip_fr_selector_fold(h_out, h_len, xg_out, target_size, sums, pptrs.size(), pptrs.data(), plens.data(), src_sizes.data(), multipliers,
                                       on_device ? 1 : 0));
}

// The gather of Varuna's round 1 (snarkvm_hip.h: snarkvm_hip_fr_witness_evals): out[k] = 0 on the input subgroup, w[k - k / ratio - 1] - x_evals[k]
// elsewhere, ratio = n / input_size; out may be x_evals.  With on_device inside a Scope the call is only enqueued.
inline void fr_witness_evals(void* out, size_t n, const DevicePoly& w, const void* x_evals, size_t input_size, bool on_device) {
    check(snarkvm_hip_fr_witness_evals(out, n, w.data, w.len, x_evals, input_size, on_device ? 1 : 0));
}

// Round 1 in lock step (snarkvm_hip.h: snarkvm_hip_fr_assignment_evals): member m of `count` reads the row vars + m * stride_vars - padded public
// input (input_size values) ++ private variables, num_vars in all - and writes the n evaluations of its assignment z to out + m * stride_out
// (strides in elements).  The inverse transform of a member is z; z div (X^input_size - 1) is w and z mod (X^input_size - 1) is x_poly.  With
// on_device inside a Scope the call is only enqueued.
inline void fr_assignment_evals(void* out, size_t n, const void* vars, size_t num_vars, size_t input_size, size_t count, size_t stride_out,
                                size_t stride_vars, bool on_device) {
    check(snarkvm_hip_fr_assignment_evals(out, n, vars, num_vars, input_size, count, stride_out, stride_vars, on_device ? 1 : 0));
}

// The sums of Varuna's round 2 in one device pass (snarkvm_hip.h: snarkvm_hip_fr_rowcheck_fold): out[i] = sum_k mu_k (a[k][i] b[k][i] - c[k][i]) and
// violations[k] = the number of i with a[k][i] b[k][i] != c[k][i], over members of n elements each.  multipliers: a.size() x 32 bytes of HOST memory,
// Montgomery form; violations: a.size() values of HOST memory, delivered when the Scope ends for a call inside one.  Either output may be nullptr
// (skipped); on_device governs out and every member vector.
inline void fr_rowcheck_fold(void* out, uint64_t* violations, size_t n, const std::vector<const void*>& a, const std::vector<const void*>& b,
                             const std::vector<const void*>& c, const void* multipliers, bool on_device) {
    if (b.size() != a.size() || c.size() != a.size()) throw std::invalid_argument("fr_rowcheck_fold: three vectors per member");
    check(snarkvm_hip_fr_rowcheck_fold(out, violations, n, a.size(), a.data(), b.data(), c.data(), multipliers, on_device ? 1 : 0));
}

// Reductions in one device pass (snarkvm_hip.h: snarkvm_hip_fr_reduce, snarkvm_hip_fr_support): the sum of a vector, the inner product of two
// (Evaluations::evaluate_with_coeffs with the Lagrange coefficients left in device memory), and the support of a coefficient vector.  `result`
// is 32 bytes of HOST memory; with on_device inside a Scope the call is only enqueued and the value arrives when the Scope ends.
inline void fr_sum(void* result, const void* a, size_t n, bool on_device) { check(snarkvm_hip_fr_reduce(SNARKVM_HIP_FR_REDUCE_SUM, result, a, nullptr, n, on_device ? 1 : 0)); }
inline void fr_inner_product(void* result, const void* a, const void* b, size_t n, bool on_device) {
    check(snarkvm_hip_fr_reduce(SNARKVM_HIP_FR_REDUCE_DOT, result, a, b, n, on_device ? 1 : 0));
}
// Evaluation of many polynomials, each at its own point, in one launch sequence (snarkvm_hip.h: snarkvm_hip_fr_evaluate): results[k] =
// polys[k](points[k]) - DensePolynomial::evaluate, the `evaluations` of a proof.  results and points: polys.size() x 32 bytes of HOST memory,
// Montgomery form, one point per member (equal points share their powers); on_device governs every polys[k].data.  No member is written;
// members may repeat and overlap.  With on_device inside a Scope the call is only enqueued and the values arrive when the Scope ends.
inline void fr_evaluate(void* results, const std::vector<DevicePoly>& polys, const void* points, bool on_device) {
    std::vector<const void*> pptrs;
    std::vector<size_t> plens;
    for (auto& p : polys) {
        pptrs.push_back(p.data);
        plens.push_back(p.len);
    }
    check(snarkvm_hip_fr_evaluate(results, pptrs.size(), pptrs.data(), plens.data(), points, on_device ? 1 : 0));
}
// trimmed_len (0: the zero vector; degree = max(trimmed_len, 1) - 1), leading_zeros (n: the zero vector), nonzero
struct FrSupport {
    uint64_t trimmed_len, leading_zeros, nonzero;
};
inline void fr_support(FrSupport& out, const void* v, size_t n, bool on_device) { check(snarkvm_hip_fr_support(&out.trimmed_len, v, n, on_device ? 1 : 0)); }

// Registered bases (an SRS resident in HBM with precomputed window tables): register once, commit per call.  `tables` x
// `window_bits` must cover 254 bits (17 x 15 for proof-sized MSMs, 12 x 22 at 2^24).  Concurrent commit() calls of proof size
// are fused inside the library (msm_batch.hip.h::msm_coalesced).
template <class Affine, class Projective>
class RegisteredBases {
public:
    RegisteredBases(const Affine* bases, size_t n, bool on_device, int tables, int window_bits) : n_(n) {
        check(snarkvm_hip_register_bases_windowed(&h_, bases, n, sizeof(Affine), on_device ? 1 : 0, tables, window_bits));
    }
    RegisteredBases(const RegisteredBases&) = delete;
    RegisteredBases& operator=(const RegisteredBases&) = delete;
    ~RegisteredBases() {
        if (h_) snarkvm_hip_free_bases(h_);
    }
    size_t size() const { return n_; }
    const snarkvm_hip_bases_t* handle() const { return h_; }  // for the raw snarkvm_hip_msm_registered* calls (device-resident scalars, batches)
    // sum_i scalars[i] * bases[offset + i]  (+ sum_j scalars[n + j] * bases[offset1 + j] when n1 > 0: KZG10's hiding term)
    Projective commit(size_t offset, size_t n, const void* scalars, bool scalars_on_device, bool scalars_montgomery = false, size_t offset1 = 0,
                      size_t n1 = 0) const {
        Projective out;
        check(snarkvm_hip_msm_registered_ex(&out, h_, offset, n, offset1, n1, scalars, scalars_on_device ? 1 : 0, scalars_montgomery ? 1 : 0, 0));
        return out;
    }

private:
    snarkvm_hip_bases_t* h_ = nullptr;
    size_t n_;
};

// A registered sparse matrix (snarkvm_hip.h: snarkvm_hip_fr_matrix_register, snarkvm_hip_fr_spmv): the CSR arrays of an R1CS matrix or of its
// transpose go to HBM once per proving key; mul() is z_M = M z (round_functions/mod.rs:131-188) or M(alpha, .) = M^T l_alpha (third.rs:303-306)
// on host or device vectors.  All n_out >= rows elements of y are written; y must not overlap x.
class RegisteredMatrix {
public:
    RegisteredMatrix(size_t rows, size_t cols, const uint64_t* row_ptr, const uint32_t* col_idx, const void* vals) : rows_(rows), cols_(cols) {
        check(snarkvm_hip_fr_matrix_register(&h_, rows, cols, row_ptr, col_idx, vals));
    }
    RegisteredMatrix(const RegisteredMatrix&) = delete;
    RegisteredMatrix& operator=(const RegisteredMatrix&) = delete;
    ~RegisteredMatrix() { snarkvm_hip_fr_matrix_free(h_); }  // waits for the device: safe with a product still enqueued in this thread's Scope
    size_t rows() const { return rows_; }
    size_t cols() const { return cols_; }
    const snarkvm_hip_fr_matrix_t* handle() const { return h_; }
    void mul(void* y, size_t n_out, const void* x, bool on_device, size_t count = 1, size_t stride_x = 0, size_t stride_y = 0) const {
        check(snarkvm_hip_fr_spmv(y, n_out, h_, x, count, stride_x, stride_y, on_device ? 1 : 0));
    }

private:
    snarkvm_hip_fr_matrix_t* h_ = nullptr;
    size_t rows_, cols_;
};

// A registered arithmetization (snarkvm_hip.h: snarkvm_hip_fr_arith_register): row, col and row_col_val of one matrix on K go to HBM once per
// proving key; matrix_sumcheck_evals() below is the fused round-4 pass over up to 16 of them (round_functions/fourth.rs:155-245).
class RegisteredArithmetization {
public:
    RegisteredArithmetization(size_t k, const void* row, const void* col, const void* row_col_val) : k_(k) {
        check(snarkvm_hip_fr_arith_register(&h_, k, row, col, row_col_val));
    }
    // from the CSR arrays of the matrix alone (snarkvm_hip.h: snarkvm_hip_fr_arith_register_csr): every device in use computes its own replica
    RegisteredArithmetization(size_t k, size_t rows, const uint64_t* row_ptr, const uint32_t* col_idx, const void* vals, uint32_t lg_constraint, uint32_t lg_variable,
                              uint32_t lg_input)
        : k_(k) {
        check(snarkvm_hip_fr_arith_register_csr(&h_, k, rows, row_ptr, col_idx, vals, lg_constraint, lg_variable, lg_input));
    }
    RegisteredArithmetization(const RegisteredArithmetization&) = delete;
    RegisteredArithmetization& operator=(const RegisteredArithmetization&) = delete;
    ~RegisteredArithmetization() { snarkvm_hip_fr_arith_free(h_); }  // waits for the device: safe with an evaluation still enqueued in this thread's Scope
    size_t size() const { return k_; }
    const snarkvm_hip_fr_arith_t* handle() const { return h_; }

private:
    snarkvm_hip_fr_arith_t* h_ = nullptr;
    size_t k_;
};
// a, b, f on K for `count` arithmetizations in one launch; an output pointer or a whole list may be null (skipped); scales = a_scale, b_scale, f_scale
inline void matrix_sumcheck_evals(const snarkvm_hip_fr_arith_t* const* ariths, size_t count, void* const* a_evals, void* const* b_evals, void* const* f_evals,
                                  const void* alpha, const void* beta, const void* scales, bool on_device) {
    check(snarkvm_hip_fr_matrix_sumcheck_evals(ariths, count, a_evals, b_evals, f_evals, alpha, beta, scales, on_device ? 1 : 0));
}

// The arithmetization on K of a CSR matrix (snarkvm_hip.h: snarkvm_hip_fr_arithmetize; matrix_evals of ahp/matrices.rs:138-195): row, col, row_col and
// row_col_val, k elements each, a null output skipped; on_device governs the CSR arrays and the outputs alike.  With on_device inside a Scope the call
// is only enqueued.
inline void fr_arithmetize(void* row, void* col, void* row_col, void* row_col_val, size_t k, size_t rows, const uint64_t* row_ptr, const uint32_t* col_idx,
                           const void* vals, uint32_t lg_constraint, uint32_t lg_variable, uint32_t lg_input, bool on_device) {
    check(snarkvm_hip_fr_arithmetize(row, col, row_col, row_col_val, k, rows, row_ptr, col_idx, vals, lg_constraint, lg_variable, lg_input, on_device ? 1 : 0));
}

}  // namespace snarkvm_hip
