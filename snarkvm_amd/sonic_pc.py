"""`SonicKZG10::{commit, combine_for_open, batch_open, open_combinations}` (algorithms/src/polycommit/sonic_pc/mod.rs:177-342, 413-473) on the gfx950 backend.

The caller side of the MSM hot path.  The reference fans the commitments of one call out over a CPU pool, one
`KZG10::commit` / `KZG10::commit_lagrange` per labelled polynomial (mod.rs:186-245), each of which re-uploads its slice of the
SRS to the GPU.  Here the committer key's base vectors - plain powers, gamma powers, shifted powers (degree bounds), the gamma
powers of every enforced bound and the Lagrange bases - live in ONE registered device vector, and a call is ONE batched device
launch (`snarkvm_hip_msm_registered_batch_ex`): instance k = (plaintext base range, hiding base range, coefficients).  The
device fuses `Fr::to_bigint` into its scalar read (kzg10/mod.rs:455-474) and runs the instances concurrently on several
streams (and devices); a degree-bounded polynomial is the same MSM starting at the shifted-powers offset
`max_bound - degree_bound` (data_structures.rs:310-331).

A linear combination of polynomials - the fold of `batch_open` over the polynomials of a query point, and every `LinearCombination`
that `open_combinations` materialises - is ONE device pass over its operands (`poly.lincomb`, `snarkvm_hip_fr_lincomb`), whatever their
number and lengths, where the reference adds term by term.

The Fiat-Shamir sponge is out of scope: `batch_open` takes the challenges it would squeeze from any object
with `squeeze_short_nonnative_field_element()`.
"""
import ctypes

import numpy as np

from . import _lib, kzg10, poly
from .kzg10 import KZG10, KZGRandomness, PCError
from .layout import G1_AFFINE, G1_PROJECTIVE

FR_MODULUS = 0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001  # r (fr.rs:137-142)
FR_ONE = np.array([0x7D1C7FFFFFFFFFF3, 0x7257F50F6FFFFFF2, 0x16D81575512C0FEE, 0x0D4BDA322BBB9A9D], dtype=np.uint64)  # Fr R (fr.rs:158-163)
# the route `SonicKZG10.evaluate_combinations_device` takes when none is named: "linear" was no slower than "fold" at any measured shape
# (3.6x - 43x faster; profiles/fr_evaluate.md holds the table and the rule that decided it)
EVALUATE_COMBINATIONS_ROUTE = "linear"


def _pts(a):
    return np.ascontiguousarray(a, dtype=G1_AFFINE).reshape(-1)


class LabeledPolynomial:
    """polycommit/sonic_pc/polynomial.rs: label, dense coefficient vector (Montgomery limbs, trimmed), optional degree bound
    and hiding bound."""

    def __init__(self, label, coeffs, degree_bound=None, hiding_bound=None):
        self.label = label
        self.coeffs = poly.trim(coeffs)
        self.degree_bound = degree_bound
        self.hiding_bound = hiding_bound

    def degree(self):  # DensePolynomial::degree: 0 for the zero polynomial
        return max(self.coeffs.shape[0] - 1, 0)

    def is_hiding(self):
        return self.hiding_bound is not None


class ResidentPolynomial:
    """A labelled polynomial whose coefficients live in device memory and stay there: `d_coeffs` is a device pointer (an int) or a
    `devmem.HipMem`, `n` the number of coefficients the caller vouches for.  Nothing is downloaded to find the degree: `n - 1` stands in
    for it as its UPPER bound in `check_degrees_and_bounds`, and every pass reads exactly n elements.  A caller whose buffer is padded (a
    full-domain product fills 2^lg elements) passes the trimmed length it already has from `snarkvm_hip_fr_support` - a padded `n` above
    `max_degree + 1` is refused with TooManyCoefficients where a trimmed one would pass."""

    def __init__(self, label, d_coeffs, n, degree_bound=None, hiding_bound=None):
        self.label = label
        self.ptr = int(getattr(d_coeffs, "ptr", d_coeffs)) if n else 0
        self.n = int(n)
        self.degree_bound = degree_bound
        self.hiding_bound = hiding_bound
        self._owner = d_coeffs  # a HipMem stays alive as long as its polynomial

    def degree(self):  # the upper bound
        return max(self.n - 1, 0)

    def is_hiding(self):
        return self.hiding_bound is not None


class LabeledEvaluations:
    """`PolynomialWithBasis::Lagrange`: evaluations over a power-of-two domain, committed in the Lagrange basis."""

    def __init__(self, label, evaluations, hiding_bound=None):
        self.label = label
        self.evaluations = np.ascontiguousarray(evaluations, dtype=np.uint64).reshape(-1, 4)
        self.degree_bound = None
        self.hiding_bound = hiding_bound

    def degree(self):
        return max(self.evaluations.shape[0] - 1, 0)


class LabeledCommitment:
    def __init__(self, label, commitment, degree_bound):
        self.label = label
        self.commitment = commitment  # G1_AFFINE record (KZGCommitment)
        self.degree_bound = degree_bound


class CommitterUnionKey:
    """sonic_pc/data_structures.rs:274-343, with every base vector registered once in HBM (one handle, recorded offsets)."""

    def __init__(self, powers_of_beta_g, powers_of_beta_times_gamma_g, shifted_powers_of_beta_g=None,
                 shifted_powers_of_beta_times_gamma_g=None, enforced_degree_bounds=None, lagrange_bases_at_beta_g=None, tables=16):
        self.powers_of_beta_g = _pts(powers_of_beta_g)
        self.powers_of_beta_times_gamma_g = _pts(powers_of_beta_times_gamma_g)
        self.shifted_powers_of_beta_g = None if shifted_powers_of_beta_g is None else _pts(shifted_powers_of_beta_g)
        self.shifted_powers_of_beta_times_gamma_g = None if shifted_powers_of_beta_times_gamma_g is None else {
            int(b): _pts(v) for b, v in shifted_powers_of_beta_times_gamma_g.items()}
        self.enforced_degree_bounds = None if enforced_degree_bounds is None else sorted(int(b) for b in enforced_degree_bounds)
        self.lagrange_bases_at_beta_g = {} if lagrange_bases_at_beta_g is None else {int(s): _pts(v) for s, v in lagrange_bases_at_beta_g.items()}
        parts, self._off = [], {}
        cursor = 0

        def place(key, arr):
            nonlocal cursor
            self._off[key] = cursor
            parts.append(arr)
            cursor += arr.shape[0]

        place("powers", self.powers_of_beta_g)
        place("gamma", self.powers_of_beta_times_gamma_g)
        if self.shifted_powers_of_beta_g is not None:
            place("shifted", self.shifted_powers_of_beta_g)
            for b, v in sorted((self.shifted_powers_of_beta_times_gamma_g or {}).items()):
                place(("shifted_gamma", b), v)
        for s, v in sorted(self.lagrange_bases_at_beta_g.items()):
            place(("lagrange", s), v)
        allpts = np.concatenate(parts)
        self._h = ctypes.c_void_p()
        _lib.check(_lib.lib().snarkvm_hip_register_bases_tables(ctypes.byref(self._h), allpts.ctypes.data, allpts.shape[0], G1_AFFINE.itemsize, 0, int(tables)))

    # ---- the views the reference hands to KZG10 (host arrays + their place in the registered vector)
    def powers(self):  # data_structures.rs:302-307
        return _PowersView(self, self._off["powers"], self.powers_of_beta_g.shape[0], self._off["gamma"], self.powers_of_beta_times_gamma_g.shape[0])

    def shifted_powers(self, degree_bound=None):  # data_structures.rs:310-331
        if self.shifted_powers_of_beta_g is None or self.shifted_powers_of_beta_times_gamma_g is None:
            return None
        max_bound = self.enforced_degree_bounds[-1]
        if degree_bound is not None:
            assert degree_bound in self.enforced_degree_bounds
            bound, start = degree_bound, max_bound - degree_bound
        else:
            bound, start = max_bound, 0
        gam = self.shifted_powers_of_beta_times_gamma_g[bound]
        return _PowersView(self, self._off["shifted"] + start, self.shifted_powers_of_beta_g.shape[0] - start, self._off[("shifted_gamma", bound)], gam.shape[0])

    def lagrange_basis(self, size):  # data_structures.rs:335-341
        if size not in self.lagrange_bases_at_beta_g:
            return None
        return _PowersView(self, self._off[("lagrange", size)], size, self._off["gamma"], self.powers_of_beta_times_gamma_g.shape[0])

    def close(self):
        if self._h:
            _lib.lib().snarkvm_hip_free_bases(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _PowersView:
    """kzg10::Powers / kzg10::LagrangeBasis as (offset, length) windows of the committer key's registered vector; quacks like
    snarkvm_amd.kzg10.Powers for KZG10.open."""

    def __init__(self, ck, off, n, gamma_off, gamma_n):
        self._h = ck._h
        self.off, self.n, self._gamma_offset, self.gamma_n = off, n, gamma_off, gamma_n
        self.powers_of_beta_times_gamma_g = np.empty(gamma_n, dtype=np.uint8)  # only its length is consulted (check_hiding_bound)

    def size(self):
        return self.n


def check_degrees_and_bounds(max_degree, enforced_degree_bounds, p):
    """kzg10/mod.rs:428-452."""
    bound = p.degree_bound
    if bound is None:
        return
    if enforced_degree_bounds is None or bound not in enforced_degree_bounds:
        raise PCError(f"UnsupportedDegreeBound({bound})")
    if bound < p.degree() or bound > max_degree:
        raise PCError(f"IncorrectDegreeBound: poly_degree {p.degree()}, degree_bound {bound}, max_degree {max_degree}, label {p.label}")


class SonicKZG10:
    @staticmethod
    def commit(max_degree, ck, polynomials, rng=None):
        """sonic_pc/mod.rs:177-257.  polynomials: LabeledPolynomial / LabeledEvaluations; rng(k) -> k random Fr elements as (k, 4)
        Montgomery limbs (required when a polynomial is hiding).  Returns ([LabeledCommitment], [KZGRandomness]), in input order.
        All commitments of the call are ONE batched device launch."""
        items = list(polynomials)
        if items and all(isinstance(p, ResidentPolynomial) for p in items):
            return SonicKZG10.commit_resident(max_degree, ck, items)
        off0, n0, off1, n1, scal, rands = [], [], [], [], [], []
        for p in items:
            check_degrees_and_bounds(max_degree, ck.enforced_degree_bounds, p)
            if isinstance(p, LabeledEvaluations):
                n = p.evaluations.shape[0]
                size = 1
                while size < n:
                    size <<= 1
                view = ck.lagrange_basis(size)
                if view is None:
                    raise PCError(f"UnsupportedLagrangeBasisSize({size})")
                if size != n:  # KZG10::commit_lagrange: evaluations.len().next_power_of_two() must be the basis size
                    raise PCError("LagrangeBasisSizeIsIncorrect")
                lz, plain = 0, p.evaluations
            else:
                view = ck.shifted_powers(p.degree_bound) if p.degree_bound is not None else ck.powers()
                if view is None:
                    raise PCError(f"UnsupportedDegreeBound({p.degree_bound})")
                if p.coeffs.shape[0] and p.degree() + 1 > view.size():  # check_degree_is_too_large (kzg10/mod.rs:407-415)
                    raise PCError(f"TooManyCoefficients: {p.degree() + 1} > {view.size()}")
                nz = np.nonzero(p.coeffs.any(axis=1))[0]  # skip_leading_zeros_and_convert_to_bigints (kzg10/mod.rs:455-467)
                lz, plain = (0, p.coeffs[:0]) if nz.size == 0 else (int(nz[0]), p.coeffs[int(nz[0]):])
            randomness = KZGRandomness.empty()
            if p.hiding_bound is not None:
                if rng is None:
                    raise PCError("MissingRng")
                randomness = KZGRandomness.rand(p.hiding_bound, rng)  # degree hiding_bound + 1 (data_structures.rs:351-356)
                kzg10.check_hiding_bound(randomness.degree(), view.gamma_n)  # kzg10/mod.rs:417-427
            blind = randomness.blinding_polynomial
            off0.append(view.off + lz)
            n0.append(plain.shape[0])
            off1.append(view._gamma_offset)
            n1.append(blind.shape[0])
            scal.append(np.ascontiguousarray(np.concatenate([plain, blind]) if blind.shape[0] else plain))
            rands.append(randomness)
        k = len(items)
        outs = np.zeros(k, dtype=G1_PROJECTIVE)
        if k:
            arr = lambda v: (ctypes.c_size_t * k)(*v)  # noqa: E731
            ptrs = (ctypes.c_void_p * k)(*[s.ctypes.data for s in scal])
            _lib.check(_lib.lib().snarkvm_hip_msm_registered_batch_ex(outs.ctypes.data, ck._h, k, arr(off0), arr(n0), arr(off1), arr(n1), ptrs, 0, 1, 0))
        affine = kzg10.to_affine(outs) if k else np.zeros(0, dtype=G1_AFFINE)
        return [LabeledCommitment(p.label, affine[i], p.degree_bound) for i, p in enumerate(items)], rands

    @staticmethod
    def commit_resident(max_degree, ck, polynomials):
        """`commit` over non-hiding `ResidentPolynomial`s (what `commit` hands a list made of them alone): the supports of all of them in one
        scope of its own (`snarkvm_hip_fr_support`: trimmed length for check_degree_is_too_large, leading zeros skipped by offset), then ONE
        batched MSM over the registered powers with the coefficients read where they live.  Refused inside a caller's scope."""
        from . import plugin

        L = _lib.lib()
        if L.snarkvm_hip_scope_stream():
            raise PCError("commit_resident: the supports of the polynomials are needed at once - not inside a scope")
        items = list(polynomials)
        views = []
        for p in items:
            check_degrees_and_bounds(max_degree, ck.enforced_degree_bounds, p)
            if p.hiding_bound is not None:
                raise PCError(f"commit_resident: {p.label} is hiding - commit its downloaded coefficients with an rng")
            view = ck.shifted_powers(p.degree_bound) if p.degree_bound is not None else ck.powers()
            if view is None:
                raise PCError(f"UnsupportedDegreeBound({p.degree_bound})")
            views.append(view)
        anchor = next((p.ptr for p in items if p.n), 0)
        if anchor:
            _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(anchor)))
        try:
            supports = [plugin.fr_support_device(p.ptr, p.n) if p.n else np.zeros(3, dtype=np.uint64) for p in items]
        finally:
            if anchor:
                _lib.check(L.snarkvm_hip_scope_end())
        k = len(items)
        off0, n0, ptrs = [], [], []
        for p, view, s in zip(items, views, supports):
            lz, plain = kzg10.resident_range(int(s[0]), int(s[1]), view.size())
            off0.append(view.off + lz), n0.append(plain), ptrs.append((p.ptr + 32 * lz) if plain else anchor)  # an empty instance reads nothing
        outs = np.zeros(k, dtype=G1_PROJECTIVE)
        if k:
            arr = lambda v: (ctypes.c_size_t * k)(*v)  # noqa: E731
            _lib.check(L.snarkvm_hip_msm_registered_batch_ex(outs.ctypes.data, ck._h, k, arr(off0), arr(n0), arr([v._gamma_offset for v in views]), arr([0] * k),
                                                             (ctypes.c_void_p * k)(*ptrs), 1, 1, 0))
        affine = kzg10.to_affine(outs) if k else np.zeros(0, dtype=G1_AFFINE)
        return [LabeledCommitment(p.label, affine[i], p.degree_bound) for i, p in enumerate(items)], [KZGRandomness.empty() for _ in items]

    @staticmethod
    def combine_polynomials(coeffs_polys_rands):
        """sonic_pc/mod.rs:548-564: sum_i coeff_i * poly_i and the same combination of the blinding polynomials, one device pass each."""
        items = list(coeffs_polys_rands)
        coeffs = [c for c, _, _ in items]
        combined_poly = poly.lincomb(coeffs, [p for _, p, _ in items])
        combined_rand = KZGRandomness(poly.lincomb(coeffs, [r.blinding_polynomial for _, _, r in items]))
        return combined_poly, combined_rand

    @staticmethod
    def combine_for_open(max_degree, ck, labeled_polynomials, rands, fs_rng):
        """sonic_pc/mod.rs:259-282: one challenge per polynomial, squeezed in order."""
        polys, rands = list(labeled_polynomials), list(rands)
        if len(polys) != len(rands):
            raise PCError("length mismatch")
        to_combine = []
        for p, r in zip(polys, rands):
            check_degrees_and_bounds(max_degree, ck.enforced_degree_bounds, p)
            to_combine.append((fs_rng.squeeze_short_nonnative_field_element(), p.coeffs, r))
        return SonicKZG10.combine_polynomials(to_combine)

    @staticmethod
    def batch_open(max_degree, ck, labeled_polynomials, query_set, rands, fs_rng):
        """sonic_pc/mod.rs:286-342.  query_set: iterable of (label, (point_name, point)); returns the KZGProofs in the order of
        the sorted point names (the reference iterates a BTreeMap)."""
        polys, rands = list(labeled_polynomials), list(rands)
        if len(polys) != len(rands):
            raise PCError("length mismatch")
        poly_rand = {p.label: (p, r) for p, r in zip(polys, rands)}
        query_to_labels = {}
        for label, (point_name, point) in query_set:
            entry = query_to_labels.setdefault(point_name, (point, set()))
            entry[1].add(label)
        proofs = []
        for point_name in sorted(query_to_labels):
            point, labels = query_to_labels[point_name]
            qp, qr = [], []
            for label in sorted(labels):
                if label not in poly_rand:
                    raise PCError(f"MissingPolynomial {{ label: {label} }}")
                qp.append(poly_rand[label][0])
                qr.append(poly_rand[label][1])
            polynomial, rand = SonicKZG10.combine_for_open(max_degree, ck, qp, qr, fs_rng)
            fs_rng.squeeze_short_nonnative_field_element()  # `_randomizer` (mod.rs:331)
            proofs.append(KZG10.open(_OpenPowers(ck.powers()), polynomial, point, rand))
        return proofs

    @staticmethod
    def open_combinations(max_degree, ck, linear_combinations, polynomials, rands, query_set, fs_rng):
        """sonic_pc/mod.rs:413-473: every linear combination becomes a labelled polynomial (and its randomness) - `ONE` terms are not
        committed to and skipped; a degree-bounded polynomial may only stand alone, with coefficient one; the hiding bound is the largest
        of the terms' - and the lot is opened with `batch_open`.  Returns its proofs (`BatchLCProof.proof`)."""
        polys, rands = list(polynomials), list(rands)
        if len(polys) != len(rands):
            raise PCError("length mismatch")
        label_map = {p.label: (p, r) for p, r in zip(polys, rands)}
        lc_polynomials, lc_randomness = [], []
        for lc in linear_combinations:
            coeffs, members, degree_bound, hiding_bound = _lc_members(lc, label_map)
            lc_polynomials.append(LabeledPolynomial(lc.label, poly.lincomb(coeffs, [p.coeffs for p, _ in members]), degree_bound, hiding_bound))
            lc_randomness.append(KZGRandomness(poly.lincomb(coeffs, [r.blinding_polynomial for _, r in members])))
        return SonicKZG10.batch_open(max_degree, ck, lc_polynomials, query_set, lc_randomness, fs_rng)

    @staticmethod
    def evaluate_polynomials_device(polynomials, query_set):
        """The `evaluations` a proof carries (snark/varuna/varuna.rs:583-592, for the labels that are polynomials: g_1 at beta, g_a, g_b, g_c per
        circuit at gamma) over `ResidentPolynomial`s: query_set holds (label, (point_name, point)) -> {(label, point_name): (4,) Montgomery
        limbs}, all from ONE `snarkvm_hip_fr_evaluate` call - every coefficient read once, the powers of a point shared by the polynomials
        queried at it.  A label that is not among the polynomials raises MissingEval(label).  Refused inside a caller's scope."""
        from . import plugin

        if _lib.lib().snarkvm_hip_scope_stream():
            raise PCError("evaluate_polynomials_device: the values are needed at once - not inside a scope")
        by_label = {p.label: p for p in polynomials}
        keys, members, points = [], [], []
        for label, (point_name, point) in query_set:
            if label not in by_label:
                raise PCError(f"MissingEval({label})")
            keys.append((label, point_name))
            members.append(by_label[label])
            points.append(np.ascontiguousarray(point, dtype=np.uint64).reshape(4))
        if not keys:
            return {}
        values = plugin.fr_evaluate_device([p.ptr if p.n else None for p in members], [p.n for p in members], np.stack(points))
        return {key: values[i].copy() for i, key in enumerate(keys)}

    @staticmethod
    def evaluate_combinations_device(linear_combinations, polynomials, query_set, route=None):
        """The loop of snark/varuna/varuna.rs:583-590 (`get_lc_eval`, ahp/ahp.rs:469-487) over `ResidentPolynomial`s: the value of every queried
        linear combination at its point, -> {(label, point_name): (4,) Montgomery limbs}; a `ONE` term adds its coefficient on the host
        (ahp.rs:480-484).  Refused inside a caller's scope.  Two routes to the same bytes:
          route="fold":   one `snarkvm_hip_fr_open_fold` without a quotient per (combination, point) - the combination is never materialised -
                          all enqueued in one scope of its own, the values read when it ends.
          route="linear": evaluation is linear, lc(z) = sum_k a_k p_k(z): the distinct (member, point) pairs of every queried combination go
                          through ONE `snarkvm_hip_fr_evaluate` call - each read once, coalesced - and the few values are combined on the
                          host, exactly.
        route=None takes EVALUATE_COMBINATIONS_ROUTE: "linear", which the measurement chose (profiles/fr_evaluate.md: device time 58 us
        against 689 us for the 4 combinations over 10 members of a gamma point at 2^17 coefficients, 222 against 811 us at 2^20; the host
        combination, 0.2 - 0.4 ms of Python integers for 10 - 28 members, is not in these figures and leaves it ahead at every shape).
        Measured for the fold route (profiles/fr_open_fold.md): for a single member it takes 0.75 - 0.81 of the time of `fr_divide_by_linear`
        without a quotient; for the 10 members of a gamma point at 2^17 coefficients it LOSES to materialising the combination with
        `fr_lincomb` and evaluating that (0.69 of its speed): without a quotient buffer the combination is formed inside the sweep, 32
        coefficients to a thread, and those reads do not coalesce.  That loss belongs to the sweep, not to the task: the linear route needs
        neither the sweep nor the intermediate vector."""
        from . import plugin

        route = EVALUATE_COMBINATIONS_ROUTE if route is None else route
        if route not in ("fold", "linear"):
            raise ValueError("route must be 'fold' or 'linear'")
        L = _lib.lib()
        if L.snarkvm_hip_scope_stream():
            raise PCError("evaluate_combinations_device: the values are needed at once - not inside a scope")
        by_label = {p.label: p for p in polynomials}
        lc_by_label = {lc.label: lc for lc in linear_combinations}
        jobs = []
        for label, (point_name, point) in query_set:
            if label not in lc_by_label:
                raise PCError(f"MissingEval({label})")
            lc = lc_by_label[label]
            constant, coeffs, members = None, [], []
            for coeff, term in lc.iter():
                if term is ONE:
                    constant = _fr_add(constant, coeff)
                    continue
                if term not in by_label:
                    raise PCError(f"MissingEval(Missing {term} for {lc.label})")
                coeffs.append(coeff)
                members.append(by_label[term])
            jobs.append(((label, point_name), point, constant, coeffs, members))
        if route == "linear":
            pairs, d_polys, lens, points = {}, [], [], []  # (label, the point's bytes) -> its row in the one call
            for _, point, _, _, members in jobs:
                z = np.ascontiguousarray(point, dtype=np.uint64).reshape(4)
                for p in members:
                    if p.n and (p.label, z.tobytes()) not in pairs:
                        pairs[(p.label, z.tobytes())] = len(d_polys)
                        d_polys.append(p.ptr), lens.append(p.n), points.append(z)
            vals = plugin.fr_evaluate_device(d_polys, lens, np.stack(points)) if d_polys else None
            out = {}
            for key, point, constant, coeffs, members in jobs:
                zb = np.ascontiguousarray(point, dtype=np.uint64).reshape(4).tobytes()
                acc = None
                for a, p in zip(coeffs, members):
                    if p.n:
                        acc = _fr_add(acc, _fr_mul(a, vals[pairs[(p.label, zb)]]))
                out[key] = _fr_add(acc, constant)
            return out
        anchor =next((p.ptr for _, _, _, _, ms in jobs for p in ms if p.n), 0)
        values = []
        if anchor:
            _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(anchor)))
        try:
            for _, point, _, coeffs, members in jobs:
                n = max([p.n for p in members] + [0])
                values.append(plugin.fr_open_fold_device(None, n, [p.ptr for p in members], [p.n for p in members], coeffs, point) if n else None)
        finally:
            if anchor:
                _lib.check(L.snarkvm_hip_scope_end())
        return {key: _fr_add(None if v is None else v[0], constant) for (key, _, constant, _, _), v in zip(jobs, values)}

    @staticmethod
    def open_combinations_device(max_degree, ck, linear_combinations, polynomials, rands, query_set, fs_rng):
        """`open_combinations` over `ResidentPolynomial`s: the same proofs as `open_combinations` on the downloaded polynomials - the same errors,
        the same hiding-bound rule, point names and the labels of a point in sorted order, the same challenges squeezed in the same order (one
        per combination of a point, then the unused `_randomizer`) - without materialising a combination.  Per point the challenges are folded
        into the members' coefficients on the host (sum_lc xi_lc sum_k a_(lc,k) p_k = sum_k (sum_lc xi_lc a_(lc,k)) p_k, exact), ONE
        `snarkvm_hip_fr_open_fold` writes the witness into a buffer of this call and a `snarkvm_hip_fr_support` of it is left pending, all
        points in one scope; when it ends the witnesses pass check_degree_is_too_large and are committed in ONE batched MSM over the
        registered powers, leading zeros skipped by offset.  The blinding side (hiding_bound + 1 coefficients) runs on host operands as in
        `open_combinations`.  Refused inside a caller's scope."""
        from . import plugin
        from .devmem import HipMem

        L = _lib.lib()
        if L.snarkvm_hip_scope_stream():
            raise PCError("open_combinations_device: the supports of the witnesses are needed at once - not inside a scope")
        polys, rands = list(polynomials), list(rands)
        if len(polys) != len(rands):
            raise PCError("length mismatch")
        label_map = {p.label: (p, r) for p, r in zip(polys, rands)}
        lcs = {}
        for lc in linear_combinations:
            coeffs, members, degree_bound, _hiding_bound = _lc_members(lc, label_map)
            for p, _ in members:
                if p.n > max_degree + 1:
                    raise PCError(f"TooManyCoefficients: {p.n} > {max_degree + 1} (label {p.label}; pass the trimmed length)")
            lcs[lc.label] = (lc, coeffs, members, degree_bound)
        query_to_labels = {}
        for label, (point_name, point) in query_set:
            query_to_labels.setdefault(point_name, (point, set()))[1].add(label)
        view = _OpenPowers(ck.powers())
        # ---- per point: the challenges, the folded coefficients and the blinding side (host)
        points = []
        for point_name in sorted(query_to_labels):
            point, labels = query_to_labels[point_name]
            folded, rand_terms = {}, []
            for label in sorted(labels):
                if label not in lcs:
                    raise PCError(f"MissingPolynomial {{ label: {label} }}")
                lc, coeffs, members, degree_bound = lcs[label]
                # the combination as a labelled polynomial: only its bound and the upper bound of its degree are consulted
                check_degrees_and_bounds(max_degree, ck.enforced_degree_bounds, ResidentPolynomial(lc.label, 0, max([p.n for p, _ in members] + [0]), degree_bound))
                xi = fs_rng.squeeze_short_nonnative_field_element()
                for a, (p, r) in zip(coeffs, members):
                    c = _fr_mul(xi, a)
                    entry = folded.setdefault(p.label, [p, None])
                    entry[1] = _fr_add(entry[1], c)
                    rand_terms.append((c, r.blinding_polynomial))
            fs_rng.squeeze_short_nonnative_field_element()  # `_randomizer` (mod.rs:331)
            rand = KZGRandomness(poly.lincomb([c for c, _ in rand_terms], [b for _, b in rand_terms]))
            hiding_witness = poly.divide_by_linear(rand.blinding_polynomial, point)[0] if rand.is_hiding() else None
            random_v, blind = kzg10.hiding_side(view, point, rand, hiding_witness)
            members = [p for p, _ in folded.values()]
            n = max([p.n for p in members] + [0])
            points.append({"point": point, "members": members, "coeffs": [c for _, c in folded.values()], "n": n, "random_v": random_v, "blind": blind,
                           "quot": HipMem(32 * max(1, n + blind.shape[0]))})
        # ---- one scope: a fused fold-and-divide and a pending support per point
        anchor = next((pt["quot"].ptr for pt in points), 0)
        if anchor:
            _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(anchor)))
        try:
            for pt in points:
                pt["support"] = np.zeros(3, dtype=np.uint64)
                if pt["n"]:
                    plugin.fr_open_fold_device(pt["quot"].ptr, pt["n"], [p.ptr for p in pt["members"]], [p.n for p in pt["members"]], pt["coeffs"], pt["point"],
                                               remainder=False)
                    pt["support"] = plugin.fr_support_device(pt["quot"].ptr, pt["n"])
        finally:
            if anchor:
                _lib.check(L.snarkvm_hip_scope_end())
        # ---- one batched MSM: witness coefficients over powers[lz ..), the hiding witness (uploaded right behind them) over the gamma powers
        k = len(points)
        off0, n0, off1, n1, ptrs = [], [], [], [], []
        for pt in points:
            trimmed_len, lz = int(pt["support"][0]), int(pt["support"][1])
            if trimmed_len and trimmed_len + 1 > view.size():  # KZG10::open's own check on the combination (mod.rs:310): one coefficient more than its witness
                raise PCError(f"TooManyCoefficients: {trimmed_len + 1} > {view.size()}")
            lz, plain = kzg10.resident_range(trimmed_len, lz, view.size())
            if pt["blind"].shape[0]:
                pt["quot"].upload(pt["blind"], 32 * (lz + plain))
            off0.append(view._view.off + lz), n0.append(plain), off1.append(view._gamma_offset), n1.append(pt["blind"].shape[0])
            ptrs.append(pt["quot"].ptr + 32 * lz)
        outs = np.zeros(k, dtype=G1_PROJECTIVE)
        if k:
            arr = lambda v: (ctypes.c_size_t * k)(*v)  # noqa: E731
            _lib.check(L.snarkvm_hip_msm_registered_batch_ex(outs.ctypes.data, ck._h, k, arr(off0), arr(n0), arr(off1), arr(n1), (ctypes.c_void_p * k)(*ptrs), 1, 1, 0))
        affine = kzg10.to_affine(outs) if k else np.zeros(0, dtype=G1_AFFINE)
        for pt in points:
            pt["quot"].free()
        return [kzg10.KZGProof(affine[i], pt["random_v"]) for i, pt in enumerate(points)]


class _One:
    """`LCTerm::One` (data_structures.rs:455-462): the constant term, which is not committed to.  Sorts before every label."""

    def __repr__(self):
        return "1"


ONE = _One()


class LinearCombination:
    """sonic_pc/data_structures.rs:525-576: a labelled map term -> coefficient, the term a polynomial label or `ONE`, the coefficient
    (4,) Montgomery limbs.  `new` merges equal terms (a sum that comes to zero stays, as in the reference); `add` also drops a term
    whose coefficient has become zero."""

    def __init__(self, label, terms=()):
        self.label = label
        self.terms = {}
        for c, t in terms:
            self.terms[t] = _fr_add(self.terms.get(t), c)

    @classmethod
    def empty(cls, label):
        return cls(label)

    @classmethod
    def new(cls, label, terms):
        return cls(label, terms)

    def add(self, c, t):
        self.terms[t] = _fr_add(self.terms.get(t), c)
        if not self.terms[t].any():
            del self.terms[t]
        return self

    def is_empty(self):
        return not self.terms

    def __len__(self):
        return len(self.terms)

    def iter(self):
        """(coefficient, term) in the order of the reference's BTreeMap: `ONE` first, then the labels."""
        for t in sorted(self.terms, key=lambda t: (t is not ONE, "" if t is ONE else t)):
            yield self.terms[t], t


def _lc_members(lc, label_map):
    """The terms of one linear combination as `open_combinations` takes them (sonic_pc/mod.rs:427-447): -> (coefficients, [(polynomial,
    randomness)], degree bound, hiding bound).  `ONE` terms are not committed to and skipped; a degree-bounded polynomial may only stand
    alone, with coefficient one; the hiding bound is the largest of the terms'."""
    coeffs, members = [], []
    degree_bound = hiding_bound = None
    for coeff, term in lc.iter():
        if term is ONE:
            continue
        if term not in label_map:
            raise PCError(f"MissingPolynomial {{ label: {term} }}")
        cur_poly, cur_rand = label_map[term]
        if cur_poly.degree_bound is not None:
            if len(lc) != 1:
                raise PCError(f"EquationHasDegreeBounds({lc.label})")
            if not np.array_equal(coeff, FR_ONE):
                raise PCError(f"Coefficient must be one for degree-bounded equations ({lc.label})")
            degree_bound = cur_poly.degree_bound
        if cur_poly.hiding_bound is not None:  # Some(_) > None
            hiding_bound = cur_poly.hiding_bound if hiding_bound is None else max(hiding_bound, cur_poly.hiding_bound)
        coeffs.append(coeff)
        members.append((cur_poly, cur_rand))
    return coeffs, members, degree_bound, hiding_bound


def _fr_limbs(x):
    return sum(int(w) << (64 * i) for i, w in enumerate(np.asarray(x, dtype=np.uint64).reshape(4)))


def _fr_mul(a, b):
    """a * b in Fr on (4,) Montgomery limbs: (a R)(b R) R^-1 = a b R, R = 2^256."""
    s = _fr_limbs(a) * _fr_limbs(b) * pow(1 << 256, -1, FR_MODULUS) % FR_MODULUS
    return np.array([(s >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def _fr_add(a, b):
    """a + b in Fr on (4,) Montgomery limbs (the Montgomery form is linear); a = None counts as zero."""
    val = lambda x: 0 if x is None else sum(int(w) << (64 * i) for i, w in enumerate(np.asarray(x, dtype=np.uint64).reshape(4)))  # noqa: E731
    s = (val(a) + val(b)) % FR_MODULUS
    return np.array([(s >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


class _OpenPowers:
    """Adapter: KZG10.open (snarkvm_amd.kzg10) addresses `powers._h` from offset `lz` and the gamma powers at `_gamma_offset`."""

    def __init__(self, view):
        self._view = view
        self._h = view._h
        self._gamma_offset = view._gamma_offset
        self.powers_of_beta_times_gamma_g = view.powers_of_beta_times_gamma_g
        if view.off != 0:
            raise PCError("the plain powers must start the registered vector")

    def size(self):
        return self._view.size()
