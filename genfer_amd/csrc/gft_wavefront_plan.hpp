// Which persistent wavefront of gft_div2d.hip runs a division / log / exp recurrence in one launch, and with which grid,
// workspace and geometry.  The one place that decides it: Ops<E>::recur_wavefront allocates what the plan asks for and
// K<E>::recur_wavefront launches it.  No HIP here, so that a plain C++ compiler can check the selection
// (tests/wavefront_plan_check.cpp).
#pragma once
#include <algorithm>
#include <cstddef>

namespace gft {

// The kernels' arguments (k_div_wavefront / k_div_wavefront_q, k_rows_wavefront, k_seg_wavefront: see there).
struct DivWfArgs {
    int L;                    // leading axes (tasks); the last axis is the row
    unsigned n[3], m[3], xn[3];   // extents of res / ys / xs on the leading axes
    unsigned nr, mr, xnr;     // row lengths
    size_t rstr[3], ystr[3], xstr[3];  // strides of the leading axes (rows are contiguous)
    unsigned ntasks;
    unsigned* flags;          // [rows] row done; zeroed before the launch
    unsigned* counter;        // next task; zeroed before the launch
    // log_mode (mt:1335-1386): res = log(xs) for the slabs k0 >= 1 (slab 0, a log one dimension down, is the caller's).
    //   level 0:  S = sum_{j0 = max(k0 + 1 - xn0, 1)}^{k0 - 1} sum_{j' lexicographic} rowproduct(xs[k0 - j0, j'], j0 * res[j0, k - j'])
    //             r = (-S) + k0 * xs[K]
    //   levels >= 1 and the row division: the division of the slab by xs[0] — as above with ys = xs[0], on the rows q of
    //             the slab's own quotient (kept in `qb`); finally res[K] = q / k0.
    // log_mode == 2: res = exp(xs) for the slabs k0 >= 1 (mt:1271-1300; slab 0, an exp one dimension down, is the caller's):
    //   res[K] = ( sum_{j0 = 1}^{min(k0, xn0 - 1)} sum_{j' lexicographic} rowproduct(j0 * xs[j0, j'], res[k0 - j0, k - j']) ) / k0
    int log_mode;
    int rev;                  // log_mode 2: the source SLABS in descending j0 — the order in which they become available (1e-10 contract,
                              // see k_rows_wavefront); set by the caller where it would otherwise take the right-looking tiled form
    const unsigned* order;    // task t works on row order[t] of the task rows (anti-diagonal order, see dwf_order); null: t
    int pack;                 // rows <= 32: two source rows per wave
    double* qb;               // log_mode: the quotient rows before the division by k0 (same layout as res)
    size_t qbp;
};

struct RowsWfArgs {
    unsigned n0, nr, m0, mr, xn0, xnr;   // rows / row lengths of res, ys (mode 0), xs
    unsigned nseg, ntasks, first_row;
    int mode;
    unsigned* flags;                     // [n0 * nseg] segment stored; zeroed before the launch
    unsigned* counter;                   // next task; zeroed before the launch
    double* qb;                          // mode 1: the quotient rows before the division by k0
    size_t qbp;
    int rev;                             // mode 2: take the source rows in DESCENDING j0 (see k_rows_wavefront)
};

struct SegWfArgs {
    int L;
    unsigned n[3], m[3], xn[3];
    unsigned nr, mr, xnr;
    size_t rstr[3], ystr[3], xstr[3];
    unsigned nseg, sl, ntasks;    // segments per row, coefficients per segment (<= 64: rows are cut EVENLY — a 65-long row is 33 + 32, not 64 + 1)
    unsigned* flags;              // [all rows of res][nseg], zeroed before the launch
    unsigned* counter;
    int log_mode;
    const unsigned* order;        // task row t works on row order[t] of the task rows (dwf_order); null: t
    double* qb;
    size_t qbp;
};

// Waves of a workgroup of these kernels = source rows of one batch (every wave takes one source row of its task, wave 0 adds the
// batch's row products in order); the LDS stages of an interval task are twice as large, hence half as many.
constexpr unsigned WF_NW_F64 = 16, WF_NW_INTERVAL = 8;

enum WfOp { WF_DIV = 0, WF_LOG = 1, WF_EXP = 2 };  // (the kernels' mode / log_mode values)
enum WfFamily {
    WF_NONE,        // no wavefront for this shape: the caller runs the blocked recurrence
    WF_ROW,         // k_div_wavefront<E, L>: ranks 2-4, a task is a row of at most 64 coefficients
    WF_ROW_QUAD16,  // k_div_wavefront_q<L, 16>: the same for f64 rows of 33 .. 64, four source rows per wave
    WF_ROW_QUAD8,   // k_div_wavefront_q<L, 8>: f64 rows of 8 .. 32
    WF_ROWS_2D,     // k_rows_wavefront<E>: rank 2, a task is a 64-coefficient segment of a row of 65 .. 4096
    WF_SEG          // k_seg_wavefront<E, L>: ranks 3 / 4 with rows of 65 .. 4096, div and log
};

struct WfPlan {
    WfFamily family;
    int L;                           // leading axes (the kernels' template argument)
    WfOp mode;
    int rev;                         // exp: each row's source slabs in the order they become available (1e-10 contract)
    unsigned ntasks, blocks;
    unsigned first;                  // first task row on axis 0 (log / exp: slab 0 is the caller's)
    size_t flag_words;               // zeroed words the launch needs: one flag per row segment of the result, then the task counter
    bool needs_qbuf;                 // log: a tensor like the result for the slab quotients
    size_t fill_offset, fill_count;  // the elements of each plane of the result (and of the quotient buffer) that start EMPTY
    DivWfArgs row;                   // the family's geometry; the pointers in it are the launcher's
    RowsWfArgs rows;
    SegWfArgs seg;
};

// z: the result's extents, x: the dividend's (log / exp: the argument's), y: the divisor's (log / exp: x again), all of rank
// nd; for div without the axes on which all three are 1.  W: doubles per element (1 = f64, 2 = interval).  arrival_order (exp):
// the caller would otherwise take the right-looking tiled form, whose contract allows that order.
inline WfPlan plan_wavefront(WfOp op, int W, int nd, const size_t* z, const size_t* x, const size_t* y, bool arrival_order) {
    WfPlan p{};
    p.family = WF_NONE;
    if (nd < 2 || nd > 4) return p;
    size_t rows = 1, x0n = 1;  // rows of the result; coefficients of x's slab 0
    int x_axes = 0;            // x's axes of extent other than 1
    bool empty_operand = false;
    for (int i = 0; i < nd; ++i) {
        if (z[i] < (op == WF_DIV ? 1u : 2u) || z[i] > 0x7fffffffu || x[i] > z[i] || y[i] > z[i]) return p;
        empty_operand |= x[i] == 0 || y[i] == 0;
        if (i + 1 < nd) rows *= z[i];
        if (i > 0) x0n *= x[i];
        x_axes += x[i] != 1;
    }
    const size_t nr = z[nd - 1], nseg = (nr + 63) / 64;
    if (rows * nseg > 0x7fffffffu) return p;
    // log: a slab divisor xs[0] of one coefficient, or x a line, is not Div's general path (mt:1194-1231)
    if (op == WF_LOG && (x0n < 2 || x_axes < 2)) return p;
    if (empty_operand && (op != WF_DIV || nr > 64)) return p;
    if (nr > 64) {
        if (nr > 4096 || rows < 8 || (op == WF_EXP && nd > 2)) return p;
        p.family = nd == 2 ? WF_ROWS_2D : WF_SEG;
    } else {
        // (fewer rows: the blocked form's few launches per slab are cheaper than a persistent launch)
        if (nr < 2 || rows < (op == WF_DIV ? 64u : 8u)) return p;
        // four source rows per wave where a row has thousands of sources (64^3 div 4.8 -> 4.0 ms); thin or small results,
        // whose time is the chain of rows, lose to its larger batches (1000 x 32 div 6.2 -> 8.0 ms)
        p.family = W == 1 && nr >= 8 && rows >= 2048 ? (nr > 32 ? WF_ROW_QUAD16 : WF_ROW_QUAD8) : WF_ROW;
    }
    p.L = nd - 1;
    p.mode = op;
    p.rev = op == WF_EXP && arrival_order;
    p.first = op == WF_DIV ? 0 : 1;
    const size_t slab = rows / z[0], task_rows = rows - p.first * slab;
    p.ntasks = (unsigned)(task_rows * nseg);
    p.blocks = std::min(p.ntasks, 256u * 2);  // persistent workgroups (they claim tasks until none is left), two per CU
    p.flag_words = rows * nseg + 1;
    p.needs_qbuf = op == WF_LOG;
    p.fill_offset = p.first * slab * nr;
    p.fill_count = task_rows * nr;
    if (p.family == WF_ROWS_2D) {
        RowsWfArgs& g = p.rows;
        g.n0 = (unsigned)z[0];
        g.nr = (unsigned)nr;
        g.m0 = (unsigned)y[0];
        g.mr = (unsigned)y[1];
        g.xn0 = (unsigned)x[0];
        g.xnr = (unsigned)x[1];
        g.nseg = (unsigned)nseg;
        g.ntasks = p.ntasks;
        g.first_row = p.first;
        g.mode = op;
        g.rev = p.rev;
        return p;
    }
    auto fill = [&](auto& g) {  // DivWfArgs and SegWfArgs share the leading-axis geometry
        g.L = p.L;
        g.log_mode = op;
        g.ntasks = p.ntasks;
        g.nr = (unsigned)nr;
        g.mr = (unsigned)y[nd - 1];
        g.xnr = (unsigned)x[nd - 1];
        size_t rs = nr, ys = y[nd - 1], xs = x[nd - 1];
        for (int a = p.L - 1; a >= 0; --a) {
            g.n[a] = (unsigned)z[a];
            g.m[a] = (unsigned)y[a];
            g.xn[a] = (unsigned)x[a];
            g.rstr[a] = rs;
            g.ystr[a] = ys;
            g.xstr[a] = xs;
            rs *= z[a];
            ys *= y[a];
            xs *= x[a];
        }
    };
    if (p.family == WF_SEG) {
        fill(p.seg);
        p.seg.nseg = (unsigned)nseg;
        p.seg.sl = (unsigned)((nr + nseg - 1) / nseg);  // rows are cut evenly: a 65-long row is 33 + 32, not 64 + 1
    } else {
        fill(p.row);
        p.row.rev = p.rev;
        p.row.pack = 1;
    }
    return p;
}

}  // namespace gft
