// Host interpreter, part 2: the scalar `Number` types the evaluator itself computes with
// (program constants, evaluation points, moment post-processing) — F64 (src/number/f64.rs), BigFloat
// (src/number/big_float.rs) and Interval over either (src/interval.rs) — and the reference's float formatting (ryu, f64.rs:41-45).
// Tensor arithmetic never happens here; it goes through the C ABI (gfh_backend.hpp).
#pragma once
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>

#include "../gft_fmt.hpp"

namespace gfh {

using gftfmt::fmt_f64;

inline double next_up(double x) {  // f64.rs:127-147
    uint64_t bits;
    std::memcpy(&bits, &x, 8);
    if (std::isnan(x) || bits == 0x7ff0000000000000ULL) return x;
    uint64_t abs = bits & 0x7fffffffffffffffULL;
    uint64_t next = (abs == 0) ? 0x1ULL : (bits == abs ? bits + 1 : bits - 1);
    double r;
    std::memcpy(&r, &next, 8);
    return r;
}
inline double next_down(double x) {  // f64.rs:150-171
    uint64_t bits;
    std::memcpy(&bits, &x, 8);
    if (std::isnan(x) || bits == 0xfff0000000000000ULL) return x;
    uint64_t abs = bits & 0x7fffffffffffffffULL;
    uint64_t next = (abs == 0) ? 0x8000000000000001ULL : (bits == abs ? bits - 1 : bits + 1);
    double r;
    std::memcpy(&r, &next, 8);
    return r;
}

struct F64 {
    static constexpr int WIDTH = 1;
    double v = 0.0;
    F64() {}
    F64(double x) : v(x) {}
    static F64 zero() { return F64(0.0); }
    static F64 one() { return F64(1.0); }
    static F64 from_u32(uint32_t u) { return F64((double)u); }
    static F64 from_ratio(uint64_t n, uint64_t d) { return F64((double)n / (double)d); }  // f64.rs:49-51
    static F64 infinity() { return F64(std::numeric_limits<double>::infinity()); }
    static F64 nan() { return F64(std::numeric_limits<double>::quiet_NaN()); }
    bool is_zero() const { return v == 0.0; }
    bool is_one() const { return v == 1.0; }
    bool is_nan() const { return std::isnan(v); }
    bool is_finite() const { return std::isfinite(v); }
    bool is_infinite() const { return std::isinf(v); }
    F64 exp() const { return F64(std::exp(v)); }
    F64 log() const { return F64(std::log(v)); }
    F64 sqrt() const { return F64(std::sqrt(v)); }
    F64 abs() const { return F64(std::fabs(v)); }
    F64 pow(uint32_t e) const { return F64(__builtin_powi(v, (int)e)); }  // f64::powi (f64.rs:64-66)
    F64 min(const F64& o) const { return v < o.v ? *this : o; }           // f64.rs:68-74
    F64 max(const F64& o) const { return v > o.v ? *this : o; }           // f64.rs:77-83
    F64 next_up() const { return F64(gfh::next_up(v)); }
    F64 next_down() const { return F64(gfh::next_down(v)); }
    double to_f64() const { return v; }
    std::string str() const { return fmt_f64(v); }
    bool operator==(const F64& o) const { return v == o.v; }
    bool operator!=(const F64& o) const { return !(v == o.v); }
    bool operator<(const F64& o) const { return v < o.v; }
    bool operator<=(const F64& o) const { return v <= o.v; }
    bool operator>(const F64& o) const { return v > o.v; }
    bool operator>=(const F64& o) const { return v >= o.v; }
    // partial_cmp(..) != Some(Less)
    bool not_less_than(const F64& o) const { return !(v < o.v); }
    void store(double* b) const { b[0] = v; }
    static F64 load(const double* b) { return F64(b[0]); }
    void store_plane(double* d, size_t, size_t i) const { d[i] = v; }
    static F64 load_plane(const double* d, size_t, size_t i) { return F64(d[i]); }
};
inline F64 operator-(F64 a) { return F64(-a.v); }
inline F64 operator+(F64 a, F64 b) { return F64(a.v + b.v); }
inline F64 operator-(F64 a, F64 b) { return F64(a.v - b.v); }
inline F64 operator*(F64 a, F64 b) { return F64(a.v * b.v); }
inline F64 operator/(F64 a, F64 b) { return F64(a.v / b.v); }

// big_float.rs:47-51 — {factor, exponent} with the factor in +-[1, 2), or 0 / non-finite.  On the C ABI (and in tensor
// planes) a BigFloat is two doubles: the factor, then the exponent (an integral double).
struct BigFloat {
    static constexpr int WIDTH = 2;
    double f = 0.0;
    int64_t e = 0;
    BigFloat() {}
    BigFloat(double factor, int64_t exponent) : f(factor), e(exponent) {}
    // f64::powi(2.0, n as i32) as this repository lowers powi (__builtin_powi, F64::pow above): exactly 2^n for
    // -1023 <= n <= 1023, +0 below, +inf above; `as i32` truncates the i64
    static double powi2(int64_t n) { return __builtin_powi(2.0, (int)(int32_t)(uint32_t)(uint64_t)n); }
    // :24-43
    static void extract_exponent(double x, double& f, int64_t& e) {
        if (!std::isfinite(x) || x == 0.0) { f = x; e = 0; return; }
        uint64_t bits;
        std::memcpy(&bits, &x, 8);
        const int64_t ex = (int64_t)((bits >> 52) & 0x7ff) - 1023;
        if (std::fpclassify(x) == FP_SUBNORMAL) {
            const double y = x * powi2(-ex);
            std::memcpy(&bits, &y, 8);
            const int64_t ex2 = (int64_t)((bits >> 52) & 0x7ff) - 1023;
            f = y * powi2(-ex2);
            e = ex + ex2;
        } else {
            f = x * powi2(-ex);
            e = ex;
        }
    }
    static BigFloat normalize(double factor, int64_t exponent) {  // :60-75
        if (factor == 0.0) return zero();
        BigFloat r;
        extract_exponent(factor, r.f, r.e);
        r.e += exponent;
        return r;
    }
    static BigFloat zero() { return BigFloat(0.0, 0); }
    static BigFloat one() { return BigFloat(1.0, 0); }
    static BigFloat from_f64(double x) { return normalize(x, 0); }                 // :115-120
    static BigFloat from_u32(uint32_t u) { return normalize((double)u, 0); }       // :107-112
    static BigFloat from_ratio(uint64_t n, uint64_t d) { return from_f64((double)n / (double)d); }  // :141-144
    static BigFloat infinity() { return from_f64(std::numeric_limits<double>::infinity()); }
    static BigFloat nan() { return from_f64(std::numeric_limits<double>::quiet_NaN()); }
    bool is_zero() const { return f == 0.0; }
    bool is_one() const { return *this == one(); }
    bool is_nan() const { return std::isnan(f); }
    bool is_finite() const { return std::isfinite(f); }
    bool is_infinite() const { return std::isinf(f); }
    double to_f64() const { return f * powi2(e); }  // :77-80
    BigFloat exp() const {  // :158-163 (`as i64` saturates, NaN -> 0)
        const double x = f * powi2(e) * 1.4426950408889634;  // LOG2_E
        int64_t k;
        if (std::isnan(x)) k = 0;
        else if (x >= 9223372036854775807.0) k = INT64_MAX;
        else if (x <= -9223372036854775808.0) k = INT64_MIN;
        else k = (int64_t)x;
        return normalize(std::pow(2.0, x - (double)k), k);
    }
    BigFloat log() const {  // :175-180
        const double l2 = std::log2(f) + (double)e;
        return from_f64(l2 * 0.6931471805599453);  // LN_2
    }
    BigFloat pow(uint32_t k) const { return normalize(__builtin_powi(f, (int)k), e * (int64_t)k); }  // :183-188
    BigFloat abs() const { return BigFloat(std::fabs(f), e); }                                      // :207-213
    BigFloat sqrt() const {  // :217-226 (div_euclid / rem_euclid by 2)
        const int64_t q = e >= 0 ? e / 2 : -((1 - e) / 2);
        return normalize(e - 2 * q == 0 ? std::sqrt(f) : std::sqrt(f * 2.0), q);
    }
    BigFloat next_up() const { return normalize(gfh::next_up(f), e); }      // :254-257
    BigFloat next_down() const { return normalize(gfh::next_down(f), e); }  // :259-262
    // PartialOrd (:130-139): -1 less, 0 equal, 1 greater, 2 unordered.  Different exponents order by exponent alone
    // unless one side is zero.
    int cmp(const BigFloat& o) const {
        if (e == o.e || is_zero() || o.is_zero()) {
            if (f < o.f) return -1;
            if (f > o.f) return 1;
            return f == o.f ? 0 : 2;
        }
        return e < o.e ? -1 : 1;
    }
    BigFloat min(const BigFloat& o) const { return *this < o ? *this : o; }  // :190-197
    BigFloat max(const BigFloat& o) const { return *this > o ? *this : o; }  // :199-205
    std::string str() const { return fmt_f64(to_f64()); }                   // :346 (Display)
    bool operator==(const BigFloat& o) const { return f == o.f && e == o.e; }
    bool operator!=(const BigFloat& o) const { return !(*this == o); }
    bool operator<(const BigFloat& o) const { return cmp(o) == -1; }
    bool operator<=(const BigFloat& o) const { const int c = cmp(o); return c == -1 || c == 0; }
    bool operator>(const BigFloat& o) const { return cmp(o) == 1; }
    bool operator>=(const BigFloat& o) const { const int c = cmp(o); return c == 1 || c == 0; }
    bool not_less_than(const BigFloat& o) const { return !(*this < o); }
    void store(double* b) const { b[0] = f; b[1] = (double)e; }
    static BigFloat load(const double* b) { return BigFloat(b[0], (int64_t)b[1]); }
    void store_plane(double* d, size_t n, size_t i) const { d[i] = f; d[n + i] = (double)e; }
    static BigFloat load_plane(const double* d, size_t n, size_t i) { return BigFloat(d[i], (int64_t)d[n + i]); }
};
inline BigFloat operator-(BigFloat a) { return BigFloat(-a.f, a.e); }  // :332-341
inline BigFloat operator+(BigFloat a, BigFloat b) {                   // :267-276
    const BigFloat& big = a.e >= b.e ? a : b;
    const BigFloat& small = a.e >= b.e ? b : a;
    return BigFloat::normalize(big.f + small.f * BigFloat::powi2(small.e - big.e), big.e);
}
inline BigFloat operator-(BigFloat a, BigFloat b) { return a + (-b); }                                   // :289-294
inline BigFloat operator*(BigFloat a, BigFloat b) { return BigFloat::normalize(a.f * b.f, a.e + b.e); }  // :302-307
inline BigFloat operator/(BigFloat a, BigFloat b) { return BigFloat::normalize(a.f / b.f, a.e - b.e); }  // :318-323

// interval.rs:12-15, instantiated at F64 (`Interval`, --bounds) and at BigFloat (`BfInterval`, the moment
// post-processing of --big-float, main.rs:256-288).
template <class B>
struct IntervalT {
    typedef IntervalT Interval;
    typedef B Bound;
    static constexpr int WIDTH = 2 * B::WIDTH;
    B lo, hi;
    IntervalT() {}
    IntervalT(B l, B h) : lo(l), hi(h) {}
    static Interval exact(B l, B h) { return Interval(l, h); }
    static Interval precisely(B x) { return Interval(x, x); }
    static Interval widen(B l, B h) { return Interval(l.next_down(), h.next_up()); }  // :28-31
    static Interval zero() { return Interval(B::zero(), B::zero()); }
    static Interval one() { return Interval(B::one(), B::one()); }
    static Interval from_u32(uint32_t u) { return Interval(B::from_u32(u), B::from_u32(u)); }  // :80-85
    static Interval from_ratio(uint64_t n, uint64_t d) {  // number.rs:24-32 (trait default)
        Interval two32 = from_u32(UINT32_MAX) + one();
        Interval numer = from_u32((uint32_t)n) + from_u32((uint32_t)(n >> 32)) * two32;
        Interval denom = from_u32((uint32_t)d) + from_u32((uint32_t)(d >> 32)) * two32;
        return numer / denom;
    }
    static Interval infinity() { return Interval(B::infinity(), B::infinity()); }
    static Interval nan() { return Interval(B::nan(), B::nan()); }
    bool is_zero() const { return lo.is_zero() && hi.is_zero(); }
    bool is_one() const { return lo.is_one() && hi.is_one(); }
    bool is_finite() const { return lo.is_finite() && hi.is_finite(); }
    bool is_nan() const { return lo.is_nan() || hi.is_nan(); }
    bool is_infinite() const { return lo.is_infinite() || hi.is_infinite(); }
    bool contains(B x) const { return lo <= x && x <= hi; }
    Interval unite(B x) const { return Interval(lo.min(x), hi.max(x)); }  // union, :38-41
    bool extract_point(B& out) const { if (lo == hi) { out = lo; return true; } return false; }
    B center() const { return (lo + hi) / B::from_u32(2); }  // :56-58
    Interval ensure_lower_bound(B nl) const { return lo < nl ? Interval(nl, hi) : *this; }  // :62-69
    Interval ensure_upper_bound(B nh) const { return hi > nh ? Interval(lo, nh) : *this; }  // :71-78
    Interval exp() const { return is_zero() ? one() : widen(lo.exp(), hi.exp()); }
    Interval log() const { return is_one() ? zero() : widen(lo.log(), hi.log()); }
    Interval pow(uint32_t e) const {  // :278-285
        Interval r = widen(lo.pow(e), hi.pow(e));
        return contains(B::zero()) ? r.unite(B::zero()) : r;
    }
    Interval min(const Interval& o) const { return Interval(lo.min(o.lo), hi.min(o.hi)); }
    Interval max(const Interval& o) const { return Interval(lo.max(o.lo), hi.max(o.hi)); }
    Interval abs() const {
        Interval r = widen(lo.abs(), hi.abs());
        return contains(B::zero()) ? r.unite(B::zero()) : r;
    }
    Interval sqrt() const {  // :304-311
        B l = lo < B::zero() ? B::zero() : lo.sqrt();
        return widen(l, hi.sqrt());
    }
    std::string str() const { return "[" + lo.str() + ", " + hi.str() + "]"; }
    bool operator==(const Interval& o) const { return lo == o.lo && hi == o.hi; }
    bool operator!=(const Interval& o) const { return !(*this == o); }
    // PartialOrd (:242-254)
    bool operator<(const Interval& o) const { return !(lo == o.lo && hi == o.hi) && hi <= o.lo; }
    bool operator>(const Interval& o) const { return !(lo == o.lo && hi == o.hi) && !(hi <= o.lo) && lo >= o.hi; }
    bool not_less_than(const Interval& o) const { return !(*this < o); }
    void store(double* b) const { lo.store(b); hi.store(b + B::WIDTH); }
    static Interval load(const double* b) { return Interval(B::load(b), B::load(b + B::WIDTH)); }
    void store_plane(double* d, size_t n, size_t i) const { lo.store_plane(d, n, i); hi.store_plane(d + B::WIDTH * n, n, i); }
    static Interval load_plane(const double* d, size_t n, size_t i) { return Interval(B::load_plane(d, n, i), B::load_plane(d + B::WIDTH * n, n, i)); }

    friend Interval operator-(Interval a) { return Interval(-a.hi, -a.lo); }
    friend Interval operator+(Interval a, Interval b) {  // :126-139
        if (a.is_zero()) return b;
        if (b.is_zero()) return a;
        return widen(a.lo + b.lo, a.hi + b.hi);
    }
    friend Interval operator-(Interval a, Interval b) { return a + (-b); }
    friend Interval operator*(Interval a, Interval b) {  // :164-190
        if ((a.is_zero() && b.is_finite()) || (a.is_finite() && b.is_zero())) return zero();
        if (a.is_one()) return b;
        if (b.is_one()) return a;
        if ((-a).is_one()) return -b;
        if ((-b).is_one()) return -a;
        B p = a.lo * b.lo, q = a.lo * b.hi, r = a.hi * b.lo, s = a.hi * b.hi;
        return widen(p.min(q).min(r).min(s), p.max(q).max(r).max(s));
    }
    friend Interval operator/(Interval a, Interval b) {  // :199-234
        if (a.is_nan() || b.is_nan()) return nan();
        if (a.is_zero() && !b.is_zero()) return a;
        if (b.is_one()) return a;
        B lo = B::infinity(), hi = -B::infinity();
        if (b.contains(B::zero())) {
            if (B::zero() <= a.lo) hi = B::infinity(); else lo = -B::infinity();
            if (a.hi <= B::zero()) lo = -B::infinity(); else hi = B::infinity();
        }
        B p = a.lo / b.lo, q = a.lo / b.hi, r = a.hi / b.lo, s = a.hi / b.hi;
        lo = lo.min(p).min(q).min(r).min(s);
        hi = hi.max(p).max(q).max(r).max(s);
        return widen(lo, hi);
    }
};
typedef IntervalT<F64> Interval;
typedef IntervalT<BigFloat> BfInterval;

}  // namespace gfh
