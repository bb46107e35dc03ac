// TEST INFRASTRUCTURE ONLY — the CPU oracle (oracle/taylor_oracle.hpp, read-only) instantiated at the reference's
// BigFloat (src/number/big_float.rs).  TaylorPoly<S> is generic over its scalar, so this is the reference's Taylor
// algorithm over BigFloat, exported as `orcb_*` with the gft_ names (bind() in genfer_amd/taylor.py serves it) plus
// `orcb_scalar_op` for the scalar pins.  Built by the tests with g++ -O2 -std=c++17 -ffp-contract=off -shared.
//
// Scalars and tensor planes are {factor, exponent}: the factor plane, then the exponent plane (integral doubles).
// Every function cites big_float.rs lines as `bf:<lines>`.
#include <cinttypes>

#include "../oracle/orc_capi.cpp"

namespace orc {

// f64::powi(2.0, n as i32), lowered as this repository lowers f64::powi (__builtin_powi: repeated squaring, the
// reciprocal for n < 0): 2^n for -1023 <= n <= 1023, +0 below, +inf above.  `as i32` keeps the low 32 bits.
inline double bf_powi2(int64_t n) { return __builtin_powi(2.0, (int32_t)(uint32_t)(uint64_t)n); }

struct BigFloat {
    double factor = 0.0;
    int64_t exponent = 0;
    BigFloat() {}
    BigFloat(double f, int64_t e) : factor(f), exponent(e) {}

    // bf:24-43 extract_exponent
    static void extract_exponent(double f, double& out_f, int64_t& out_e) {
        if (!std::isfinite(f) || f == 0.0) {
            out_f = f;
            out_e = 0;
            return;
        }
        uint64_t bits;
        std::memcpy(&bits, &f, 8);
        int64_t e = (int64_t)((bits >> 52) & 0x7ff) - 1023;
        if (std::fpclassify(f) == FP_SUBNORMAL) {
            const double g = f * bf_powi2(-e);
            std::memcpy(&bits, &g, 8);
            const int64_t e2 = (int64_t)((bits >> 52) & 0x7ff) - 1023;
            out_f = g * bf_powi2(-e2);
            out_e = e + e2;
        } else {
            out_f = f * bf_powi2(-e);
            out_e = e;
        }
    }
    // bf:60-75 normalize: zero factors (either sign) give {+0, 0}; non-finite factors keep `exponent`
    static BigFloat normalize(double f, int64_t exponent) {
        if (f == 0.0) return zero();
        double g;
        int64_t e;
        extract_exponent(f, g, e);
        return BigFloat(g, e + exponent);
    }
    static BigFloat zero() { return BigFloat(0.0, 0); }                        // bf:84-90
    static BigFloat one() { return BigFloat(1.0, 0); }                         // bf:98-104
    static BigFloat from_u32(uint32_t u) { return normalize((double)u, 0); }   // bf:107-112
    bool is_zero() const { return factor == 0.0; }                             // bf:92-95
    bool is_one() const { return *this == one(); }                             // num_traits::One default
    double to_f64() const { return factor * bf_powi2(exponent); }              // bf:77-80
    // bf:158-163
    BigFloat exp() const {
        const double x = factor * bf_powi2(exponent) * 1.4426950408889634;  // LOG2_E
        int64_t k = 0;  // `as i64`: saturating, NaN -> 0
        if (x != x) k = 0;
        else if (x >= 9223372036854775807.0) k = INT64_MAX;
        else if (x <= -9223372036854775808.0) k = INT64_MIN;
        else k = (int64_t)x;
        return normalize(std::pow(2.0, x - (double)k), k);
    }
    // bf:175-180
    BigFloat log() const { return normalize((std::log2(factor) + (double)exponent) * 0.6931471805599453, 0); }
    bool operator==(const BigFloat& o) const { return factor == o.factor && exponent == o.exponent; }  // derived
    // bf:130-139 partial_cmp as -1 / 0 / 1, 2 = None: equal exponents, or a zero on either side, compare the factors;
    // otherwise the exponents alone decide (whatever the signs)
    int partial_cmp(const BigFloat& o) const {
        if (exponent != o.exponent && !is_zero() && !o.is_zero()) return exponent < o.exponent ? -1 : 1;
        if (factor < o.factor) return -1;
        if (factor > o.factor) return 1;
        return factor == o.factor ? 0 : 2;
    }
    BigFloat min(const BigFloat& o) const { return partial_cmp(o) == -1 ? *this : o; }  // bf:190-197
    BigFloat max(const BigFloat& o) const { return partial_cmp(o) == 1 ? *this : o; }   // bf:199-205
    BigFloat abs() const { return BigFloat(std::fabs(factor), exponent); }              // bf:207-213
    BigFloat pow(uint32_t k) const {                                                    // bf:183-188
        return normalize(__builtin_powi(factor, (int32_t)k), exponent * (int64_t)k);
    }
    // bf:217-226: div_euclid / rem_euclid by 2 (a floor division for negative exponents)
    BigFloat sqrt() const {
        int64_t q = exponent / 2, r = exponent % 2;
        if (r < 0) {
            q -= 1;
            r += 2;
        }
        return normalize(r == 0 ? std::sqrt(factor) : std::sqrt(factor * 2.0), q);
    }
    BigFloat next_up() const { return normalize(orc::next_up(factor), exponent); }      // bf:254-257
    BigFloat next_down() const { return normalize(orc::next_down(factor), exponent); }  // bf:259-262
};
inline BigFloat operator-(BigFloat a) { return BigFloat(-a.factor, a.exponent); }  // bf:332-341
// bf:267-276: "bigger" = larger exponent, self on a tie
inline BigFloat operator+(BigFloat a, BigFloat b) {
    BigFloat bigger = a, smaller = b;
    if (!(a.exponent >= b.exponent)) {
        bigger = b;
        smaller = a;
    }
    const int64_t diff = smaller.exponent - bigger.exponent;
    return BigFloat::normalize(bigger.factor + smaller.factor * bf_powi2(diff), bigger.exponent);
}
inline BigFloat operator-(BigFloat a, BigFloat b) { return a + (-b); }                                              // bf:289-294
inline BigFloat operator*(BigFloat a, BigFloat b) { return BigFloat::normalize(a.factor * b.factor, a.exponent + b.exponent); }  // bf:302-307
inline BigFloat operator/(BigFloat a, BigFloat b) { return BigFloat::normalize(a.factor / b.factor, a.exponent - b.exponent); }  // bf:318-323
// bf:344-348 Display: ryu of to_f64 (found by argument-dependent lookup from orc_capi.cpp's formatter)
inline std::string fmt_scalar(const BigFloat& s) { return ::fmt_num(s.to_f64()); }

}  // namespace orc

template <>
struct Tr<BigFloat> {
    static constexpr int W = 2;
    static BigFloat load(const double* p) { return BigFloat(p[0], (int64_t)p[1]); }
    static void store(BigFloat s, double* p) {
        p[0] = s.factor;
        p[1] = (double)s.exponent;
    }
    static BigFloat load_plane(const double* d, usize n, usize i) { return BigFloat(d[i], (int64_t)d[n + i]); }
    static void store_plane(BigFloat s, double* d, usize n, usize i) {
        d[i] = s.factor;
        d[n + i] = (double)s.exponent;
    }
};

DEFINE_API(orcb_, BigFloat)

extern "C" {
// One raw scalar operation, numbered as gfh_bigfloat_op: 0 add, 1 sub, 2 mul, 3 div, 4 neg, 5 exp, 6 log,
// 7 normalize(a.factor, a.exponent), 8 to_f64 (into out[0]), 9 sqrt, 10 next_up, 11 next_down, 12 partial_cmp (into
// out[0]), 13 min, 14 max, 15 abs, 16 pow(a, (uint32_t)b.factor).
int orcb_scalar_op(int op, const double* a, const double* b, double* out) {
    const BigFloat x = Tr<BigFloat>::load(a), y = b ? Tr<BigFloat>::load(b) : BigFloat();
    BigFloat r;
    switch (op) {
        case 0: r = x + y; break;
        case 1: r = x - y; break;
        case 2: r = x * y; break;
        case 3: r = x / y; break;
        case 4: r = -x; break;
        case 5: r = x.exp(); break;
        case 6: r = x.log(); break;
        case 7: r = BigFloat::normalize(x.factor, x.exponent); break;
        case 8:
            out[0] = x.to_f64();
            out[1] = 0.0;
            return 0;
        case 9: r = x.sqrt(); break;
        case 10: r = x.next_up(); break;
        case 11: r = x.next_down(); break;
        case 12:
            out[0] = x.partial_cmp(y);
            out[1] = 0.0;
            return 0;
        case 13: r = x.min(y); break;
        case 14: r = x.max(y); break;
        case 15: r = x.abs(); break;
        case 16: r = x.pow((uint32_t)b[0]); break;
        default: return -1;
    }
    Tr<BigFloat>::store(r, out);
    return 0;
}
}
