// Part of struct Ops<E> (included inside its body by gft_api.hip): division, exp, log (mt:406-430, 1162-1386): the recurrence drivers and their wavefront launches.
// Split out of gft_api.hip in round 6 by concern; no behavioural change (the compiler sees the same token stream).

    // ---- division (mt:1162-1231) -----------------------------------------------------------------------------
    static int nonunit_axes(const Dims& s) {
        int n = 0;
        for (size_t x : s)
            if (x != 1) n++;
        return n;
    }
    struct TiledMin {  // tiled-kernel crossover for the products issued inside this scope
        double prev;
        explicit TiledMin(double v) : prev(R.tiled_min_override) { R.tiled_min_override = v; }
        ~TiledMin() { R.tiled_min_override = prev; }
    };
    // tier-dispatched launches used by the recurrences (views carry their side)
    static void x_map_inplace(const HV& v, int op, unsigned u) {
        if (v.host) HK<E>::map_inplace(v.p, v.plane, v.numel(), op, u, Scalar2{0, 0});
        else K<E>::map_inplace(R.stream, v.p, v.plane, v.numel(), op, u, Scalar2{0, 0});
    }
    static void x_block_op(const HV& dst, const HV& src, int op, unsigned u) {
        Dims keep = collapse_mask({&dst.shape}, false);
        if (dst.host) HK<E>::block_op(dview(dst, &keep), dview(src, &keep), op, u);
        else K<E>::block_op(R.stream, dview(dst, &keep), dview(src, &keep), op, u);
    }
    static void x_set_scalar(const HV& dst, Scalar2 v) {
        if (dst.host) E::st(dst.p, dst.plane, 0, E::from(v));
        else K<E>::set_small(R.stream, dst.p, dst.plane, 1, v, v);
    }
    static void copy_planes(bool host, double* dst, size_t dplane, const double* src, size_t splane, size_t n) {
        copy_elems(host, dst, src, n);
        if (W == 2) copy_elems(host, dst + dplane, src + splane, n);
    }
    // z[0..m) += a (*) b for the m slabs that follow a slab the recurrence has just finalised (right-looking update, see
    // div_rec).  Only z[0] is needed by the next step of the recurrence: it is updated on the main stream, the other m - 1
    // slabs on the side stream, overlapping the next slab's division (a single-workgroup latency chain that leaves the
    // GPU empty).  Order per slab is unchanged — slab s receives term j from bulk(j) for j < s - 1 (side stream, in
    // order), then from the critical update of step s - 1, which waits for the latest bulk first.
    static void right_update(const HV& a, const HV& b, const HV& z, size_t m) {
        TiledMin guard(R.recur_tiled_min_macs);
        // The overlap is only legal for launches that own nothing but their arguments: the reference-order kernels.  A
        // tiled product takes pooled temporaries (freed for reuse by the MAIN stream as soon as conv() returns), the
        // one conv workspace and the non-finite epoch word — shared state that two streams must not touch at once.  So
        // whenever a product of this recurrence could take the tiled kernel ("recur_tiled_min_macs" lowered, or
        // conv_mode 2) everything stays on the main stream.
        const bool may_tile = W == 1 && (R.conv_mode == 2 || (R.conv_mode == 0 && R.recur_tiled_min_macs < 1.0e299));
        if (!R.recur_overlap || !R.side || m < 2 || may_tile) {
            join_side();
            conv(a, b, z, 0, m, true, false, 0, 0, 0);
            return;
        }
        join_side();  // the previous bulk added its term to z[0] (and beyond)
        conv(a, b, z, 0, 1, true, false, 0, 0, 0);
        {
            hipStream_t ms = R.stream, ss = R.side;
            hipEvent_t ev = R.ev_main;
            enqueue_task([=] {  // slab final (+ critical update): the bulk may read it
                lq_note((hipEventRecord)(ev, ms), nullptr, "hipEventRecord (main stream)");
                lq_note((hipStreamWaitEvent)(ss, ev, 0), nullptr, "hipStreamWaitEvent (side stream)");
            });
        }
        std::swap(R.stream, R.side);
        try {
            conv(a, b, z, 1, m, true, false, 0, 0, 0);
        } catch (...) {
            std::swap(R.stream, R.side);
            throw;
        }
        std::swap(R.stream, R.side);
        {
            hipStream_t ss = R.side;
            hipEvent_t ev = R.ev_bulk;
            enqueue_task([=] { lq_note((hipEventRecord)(ev, ss), nullptr, "hipEventRecord (side stream)"); });
        }
        R.side_pending = true;
    }
    // Unwinding out of a recurrence with a bulk update in flight: its operands (rsbuf / tmp / the quotient itself) are
    // about to be released, so the side stream is drained first.
    struct SideDrain {
        ~SideDrain() {
            if (R.side_pending && std::uncaught_exceptions()) {
                launch_drain_nothrow();  // (a destructor during unwinding: a latched launch failure stays latched)
                (void)(hipStreamSynchronize)(R.side);
                R.side_pending = false;
            }
        }
    };
    // the main stream waits for everything issued on the side stream so far
    static void join_side() {
        if (!R.side_pending) return;
        {
            hipStream_t ms = R.stream;
            hipEvent_t ev = R.ev_bulk;
            enqueue_task([=] { lq_note((hipStreamWaitEvent)(ms, ev, 0), nullptr, "hipStreamWaitEvent (main stream)"); });
        }
        R.side_pending = false;
    }
    static void div_rec(const HV& xs, const HV& ys, const HV& res) {
        if (xs.numel() == 0) return;
        SideDrain drain_on_unwind;
        const bool host = res.host;
        if (res.shape.empty()) {
            if (host) E::st(res.p, res.plane, 0, E::div(E::ld(xs.p, xs.plane, 0), E::ld(ys.p, ys.plane, 0)));
            else K<E>::scalar_op(R.stream, SC_DIV, xs.p, xs.plane, ys.p, ys.plane, res.p, res.plane);
            return;
        }
        if (res.shape.size() == 1) {  // last level: fused sequential recurrence
            if (host)
                HK<E>::div_1d(xs.p, xs.plane, (unsigned)xs.shape[0], ys.p, ys.plane, (unsigned)ys.shape[0], res.p, res.plane,
                              (unsigned)res.shape[0]);
            else
                K<E>::div_1d(R.stream, xs.p, xs.plane, (unsigned)xs.shape[0], ys.p, ys.plane, (unsigned)ys.shape[0], res.p,
                             res.plane, (unsigned)res.shape[0]);
            return;
        }
        if (!host && res.shape.size() == 2 &&
            K<E>::div_2d(R.stream, xs.p, xs.plane, (unsigned)xs.shape[0], (unsigned)xs.shape[1], xs.shape[1], ys.p, ys.plane,
                         (unsigned)ys.shape[0], (unsigned)ys.shape[1], res.p, res.plane, (unsigned)res.shape[0], (unsigned)res.shape[1], 0))
            return;  // the last two axes in one launch (gft_div2d.hip), same bits
        size_t n0 = res.shape[0];
        HV y0 = ys.index0(0);
        // Device tier: RIGHT-LOOKING accumulation.  The reference forms cur = sum_{j<k} res[j] (*) ys[k-j] when it reaches
        // slab k (one product per (k, j): 64 small dependent launches a slab).  Here the quotient's own memory holds the
        // running sums: as soon as slab k is final, ONE product adds res[k] (*) ys[1..m] into the m slabs that follow.
        // Every slab still receives its terms in ascending j, each term's row products formed from zero (mt:971-982), so
        // the bits are the reference's; what changes is that a step is a product of m slabs wide — hundreds of
        // workgroups instead of four.  Steps of at least recur_tiled_min_macs multiply-adds may take the tiled kernel
        // (different summation order: 1e-10 contract), smaller ones keep the reference order.
        const bool right = !host;
        Dims rest(res.shape.begin() + 1, res.shape.end()), yrest(ys.shape.begin() + 1, ys.shape.end());
        if (right) {
            zero_elems(false, res.p, res.numel());
            if (W == 2) zero_elems(false, res.p + res.plane, res.numel());
        }
        for (size_t k = 0; k < n0; ++k) {
            HV cur = res.index0(k);
            if (!right) conv(res, ys, res, k, k + 1, false, true, 0, 1, 0);  // cur = sum_{j<k} res[j] (*) ys[k-j]
            struct Scatter {  // runs when slab k is final, whichever branch below finalised it
                const HV &res, &ys, &cur;
                const Dims &rest, &yrest;
                size_t k, n0;
                bool on;
                ~Scatter() noexcept(false) {
                    if (!on || k + 1 >= n0 || ys.shape[0] < 2 || std::uncaught_exceptions()) return;
                    const size_t m = std::min(n0 - 1 - k, ys.shape[0] - 1);
                    Dims xs1{1}, ysm{m}, zsm{m};
                    xs1.insert(xs1.end(), rest.begin(), rest.end());
                    ysm.insert(ysm.end(), yrest.begin(), yrest.end());
                    zsm.insert(zsm.end(), rest.begin(), rest.end());
                    HV xk{cur.p, res.plane, xs1, false}, ym{ys.p + prod(yrest), ys.plane, ysm, false},
                        zm{res.p + (k + 1) * prod(rest), res.plane, zsm, false};
                    right_update(xk, ym, zm, m);
                }
            } scatter{res, ys, cur, rest, yrest, k, n0, right};
            if (!host && cur.shape.size() == 2) {
                // neg, += xs[k], copy and the whole 2-d division of the slab fused into one launch
                const bool have_x = k < xs.shape[0];
                HV xk = have_x ? xs.index0(k) : HV{nullptr, 0, Dims{0, 0}, false};
                if (K<E>::div_2d(R.stream, xk.p, xk.plane, have_x ? (unsigned)xk.shape[0] : 0u, have_x ? (unsigned)xk.shape[1] : 0u,
                                 have_x ? xk.shape[1] : 0, y0.p, y0.plane, (unsigned)y0.shape[0], (unsigned)y0.shape[1], cur.p, cur.plane,
                                 (unsigned)cur.shape[0], (unsigned)cur.shape[1], 1))
                    continue;
            }
            if (!host && cur.shape.size() == 1) {
                // 2-d quotient whose rows do not fit the slab kernel: row by row, each row's neg, += xs[k], copy and 1-d
                // division in one launch
                const bool have_x = k < xs.shape[0];
                HV xk = have_x ? xs.index0(k) : HV{nullptr, 0, Dims{0}, false};
                if (K<E>::div_1d(R.stream, xk.p, xk.plane, have_x ? (unsigned)xk.shape[0] : 0u, y0.p, y0.plane, (unsigned)y0.shape[0], cur.p,
                                 cur.plane, (unsigned)cur.shape[0], 1))
                    continue;
            }
            x_map_inplace(cur, MAP_NEG, 0);
            if (k < xs.shape[0]) x_block_op(cur, xs.index0(k), BLK_ADD, 0);
            Rc<Buf> tmp = alloc_tier(host, cur.numel() * W);
            HV copy{tmp->p, cur.numel(), cur.shape, host};
            copy_planes(host, copy.p, copy.plane, cur.p, cur.plane, cur.numel());
            div_rec(copy, y0, cur);
        }
        if (right) join_side();
    }
    static P div(P self, P other) {
        broadcast(self, other);
        Dims deg = min_degrees(self, other);
        truncate_here(self, deg);
        truncate_here(other, deg);
        if (is_one(other)) return self;
        if (other.numel == 1) {
            double c[2];
            first_value(other, c);
            return map_copy(self, OP_DIV_S, c);
        }
        Dims rs = deg;
        for (size_t i = 0; i < rs.size(); ++i)
            if (other.shape[i] == 1) rs[i] = self.shape[i];
        for (size_t i = 0; i < rs.size(); ++i)
            if (rs[i] == UMAX) throw Error("div: untruncated result shape (degrees_p1 == usize::MAX)");
        const bool host = tier_host(prod(rs), self, other) && est_macs(rs, other.shape, rs) <= R.host_max_macs;
        P out = make(rs, deg, host);
        if (!host) {  // (dropped axes have extent 1 in the result, hence in both operands: shapes never exceed the result's)
            Dims keep = collapse_mask({&out.shape}, false);
            HV x{dp<E>(self), self.numel, pick(self.shape, keep), false}, y{dp<E>(other), other.numel, pick(other.shape, keep), false},
                z{dp<E>(out), out.numel, pick(out.shape, keep), false};
            if (recur_wavefront(WF_DIV, x, y, z)) return out;
        }
        div_rec(view(self, host), view(other, host), view(out, host));
        return seal(out);
    }
    // The whole recurrence in one persistent launch, the kernel and its geometry chosen by plan_wavefront (gft_wavefront_plan.hpp):
    // every result row (or 64-coefficient segment of one) a task, its terms consumed in the reference's order — or, exp with
    // `arrival_order`, in the order they become available — with dependencies through per-segment flags.  x, y, z: contiguous
    // device views of one rank (log / exp: y = x, and the slabs k0 >= 1 of z).  false: no wavefront for this shape, nothing
    // allocated or launched.
    static bool recur_wavefront(WfOp op, const HV& x, const HV& y, const HV& z, bool arrival_order = false) {
        const size_t nd = z.shape.size();
        if (!R.div_wavefront || x.shape.size() != nd || y.shape.size() != nd) return false;
        const WfPlan p = plan_wavefront(op, W, (int)nd, z.shape.data(), x.shape.data(), y.shape.data(), arrival_order);
        if (p.family == WF_NONE) return false;
        Rc<Buf> qb = p.needs_qbuf ? alloc_doubles(z.numel() * W) : Rc<Buf>();
        const size_t fl_doubles = (p.flag_words + 1) / 2 + 1;
        Rc<Buf> fl = alloc_doubles(fl_doubles);
        zero_elems(false, fl->p, fl_doubles);
        K<E>::recur_wavefront(R.stream, p, x.p, x.plane, y.p, y.plane, z.p, z.plane, qb ? qb->p : nullptr, qb ? z.numel() : 0,
                              reinterpret_cast<unsigned*>(fl->p));
        return true;
    }
    // ---- exp / log (mt:406-430, 1270-1386) ---------------------------------------------------------------------
    // xs scaled slab-wise by T::from(j) along axis 0 (mt:1308-1310): xs[j] * j
    static Rc<Buf> scaled_by_index(const HV& xs, HV* out) {
        const bool host = xs.host;
        Rc<Buf> buf = alloc_tier(host, xs.numel() * W);
        Rc<Buf> tab = cached_table(TAB_INDEX, 0, xs.shape[0], host);
        GatherArgs a;
        std::memset(&a, 0, sizeof(a));
        size_t inner = xs.numel() / std::max<size_t>(xs.shape[0], 1);
        a.out.nd = 2;
        a.out.d[0] = (unsigned)xs.shape[0];
        a.out.d[1] = (unsigned)inner;
        a.src_len[0] = a.out.d[0];
        a.src_len[1] = a.out.d[1];
        a.src_stride[0] = inner;
        a.src_stride[1] = 1;
        a.op = OP_MUL_TAB;
        a.tab_axis = 0;
        a.tab = tab->p;
        a.tab_plane = xs.shape[0];
        *out = HV{buf->p, xs.numel(), xs.shape, host};
        if (host) HK<E>::gather(xs.p, xs.plane, buf->p, xs.numel(), a);
        else K<E>::gather(R.stream, xs.p, xs.plane, buf->p, xs.numel(), a);
        return buf;
    }
    // The scalar seeds exp(xs[0]) / ln(xs[0]) (mt:1286-1289, 1336-1339; f64.rs:54-61 = the platform libm) are formed on
    // the host from the constant term — one value, SURVEY §8a row S — so that they are the same libm result whichever
    // side runs the recurrence; every coefficient operation after the seed is device (or host-tier) arithmetic.
    // The 1-d base case of exp / log on DEVICE tensors.  Its order (the newest coefficient's term first, mt:1296-1310)
    // makes it one serial chain of n^2/2 multiply-adds: a single GPU lane needs 75 ns a step (1.5 ms for a 200-long line,
    // 30 ms for 900 — slower than the CPU from ~100 coefficients on), a host core 1 ns.  Lines of 48 coefficients or more
    // therefore make the round trip: the argument line to pinned host memory, the host tier's own loop (the same functor,
    // the same bits), the result line back.  ~25 us of synchronisation against milliseconds.
    template <class F>
    static bool line_on_host(const HV& xs, const HV& res, F&& compute) {
        const size_t nxh = xs.numel(), nrh = res.numel();
        if (nrh < 48 || nrh > 65536) return false;
        std::vector<double> hx(nxh * W), hr(nrh * W);
        for (size_t pl = 0; pl < (size_t)W; ++pl)
            HIP_OK(hipMemcpyAsync(hx.data() + pl * nxh, xs.p + pl * xs.plane, sizeof(double) * nxh, hipMemcpyDeviceToHost, R.stream));
        HIP_OK(hipStreamSynchronize(R.stream));
        compute(hx.data(), nxh, hr.data(), nrh);
        for (size_t pl = 0; pl < (size_t)W; ++pl)
            HIP_OK(hipMemcpyAsync(res.p + pl * res.plane, hr.data() + pl * nrh, sizeof(double) * nrh, hipMemcpyHostToDevice, R.stream));
        HIP_OK(hipStreamSynchronize(R.stream));  // hr is pageable and dies here
        R.stats[6]++;
        return true;
    }
    static void exp_rec(const HV& xs, const HV& res, Scalar2 seed) {
        if (xs.numel() == 0) return;
        if (res.shape.empty()) {
            x_set_scalar(res, seed);
            return;
        }
        if (nonunit_axes(res.shape) == 1) {
            if (res.host) HK<E>::exp_1d(xs.p, xs.plane, (unsigned)xs.numel(), res.p, res.plane, (unsigned)res.numel(), seed);
            else if (!line_on_host(xs, res, [&](const double* hx, size_t nxh, double* hr, size_t nrh) {
                         HK<E>::exp_1d(hx, nxh, (unsigned)nxh, hr, nrh, (unsigned)nrh, seed);
                     }))
                K<E>::exp_1d(R.stream, xs.p, xs.plane, (unsigned)xs.numel(), res.p, res.plane, (unsigned)res.numel(), seed);
            return;
        }
        exp_rec(xs.index0(0), res.index0(0), seed);
        if (res.shape[0] <= 1) return;
        // below the right-looking tiled path's crossover (and for intervals at every size): the row wavefront, one launch,
        // the reference's summation order
        double total = 1.0;
        for (size_t i = 0; i < res.shape.size(); ++i) total *= 0.5 * (double)res.shape[i] * (double)std::min(xs.shape[i], res.shape[i]) + 0.5;
        const bool right_tiled = !res.host && W == 1 && R.conv_mode == 0 && R.exp_right && total >= 64.0 * R.tiled_min_macs;
        // (rank 2 with long rows: the coefficient-level wavefront keeps the reference's order AND beats the right-looking tiled
        // form — 400^2: see profiles/r04/recurrences.txt)
        // rank 2 where the right-looking tiled form would be taken: the wavefront kernels with each row's terms in the order of
        // their ARRIVAL (that form's order, same 1e-10 contract) — 400^2 62 -> 4.5 ms, 1000 x 32 10.6 -> see recurrences.txt
        const bool wf_2d = res.shape.size() == 2 && res.shape[1] <= 4096;
        if (!res.host && (!right_tiled || wf_2d) && recur_wavefront(WF_EXP, xs, xs, res, right_tiled)) return;
        HV xsc;
        Rc<Buf> hold = scaled_by_index(xs, &xsc);
        // Large f64 exponentials (their slab steps would take the tiled kernel anyway, i.e. the 1e-10 contract, not the
        // reference's summation order): RIGHT-LOOKING.  As soon as res[i] is final one wide product adds
        // (j xs[j]) (*) res[i] for j = 1..m into the m slabs that follow — 64 wide launches at full tile efficiency
        // instead of 64 single-slab launches that are all launch / reduce overhead (64^3: 15.6 -> see recurrences.txt).
        const size_t n0 = res.shape[0];
        if (right_tiled) {
            Dims rest(res.shape.begin() + 1, res.shape.end()), xrest(xs.shape.begin() + 1, xs.shape.end());
            HV tail = res.index0(1);
            zero_elems(false, tail.p, res.numel() - prod(rest));
            for (size_t i = 0; i + 1 < n0; ++i) {
                HV cur = res.index0(i);
                if (i >= 1) x_map_inplace(cur, MAP_DIV_U32, (unsigned)i);  // res[i] = acc / i: final
                if (xs.shape[0] < 2) continue;
                const size_t m = std::min(n0 - 1 - i, xs.shape[0] - 1);
                Dims xsm{m}, ys1{1}, zsm{m};
                xsm.insert(xsm.end(), xrest.begin(), xrest.end());
                ys1.insert(ys1.end(), rest.begin(), rest.end());
                zsm.insert(zsm.end(), rest.begin(), rest.end());
                HV xm{xsc.p + prod(xrest), xsc.plane, xsm, false}, yi{cur.p, res.plane, ys1, false},
                    zm{res.p + (i + 1) * prod(rest), res.plane, zsm, false};
                conv(xm, yi, zm, 0, m, true, false, 0, 0, 0);
            }
            x_map_inplace(res.index0(n0 - 1), MAP_DIV_U32, (unsigned)(n0 - 1));
            return;
        }
        for (size_t k = 1; k < n0; ++k) {
            HV cur = res.index0(k);
            conv(xsc, res, res, k, k + 1, false, true, 1, 0, 0);
            x_map_inplace(cur, MAP_DIV_U32, (unsigned)k);
        }
    }
    static Dims explog_shape(const P& a) {
        Dims rs = a.deg;
        for (size_t i = 0; i < rs.size(); ++i) {
            if (a.shape[i] == 1) rs[i] = 1;
            if (rs[i] == UMAX) throw Error("exp/log: untruncated result shape (degrees_p1 == usize::MAX)");
        }
        return rs;
    }
    static Scalar2 seed_of(const P& a, bool is_exp) {
        double c[2];
        first_value(a, c);
        typename E::V r = is_exp ? E::exp(E::from(hv(c))) : E::log(E::from(hv(c)));
        double o[2] = {0.0, 0.0};
        E::st(o, 1, 0, r);
        return Scalar2{o[0], o[1]};
    }
    static P exp(const P& a) {
        Dims rs = explog_shape(a);
        const bool host = tier_host(prod(rs), a) && est_macs(a.shape, rs, rs) <= R.host_max_macs;
        P out = make(rs, a.deg, host);
        exp_rec(view(a, host), view(out, host), seed_of(a, true));
        return seal(out);
    }

    static void log_rec(const HV& xs, const HV& res, Scalar2 seed) {
        if (xs.numel() == 0) return;
        SideDrain drain_on_unwind;
        const bool host = res.host;
        if (res.shape.empty()) {
            x_set_scalar(res, seed);
            return;
        }
        if (nonunit_axes(xs.shape) == 1) {
            if (nonunit_axes(res.shape) != 1) throw Error("log: called `Option::unwrap()` on a `None` value (mt:1346)");
            if (host) HK<E>::log_1d(xs.p, xs.plane, (unsigned)xs.numel(), res.p, res.plane, (unsigned)res.numel(), seed);
            else if (!line_on_host(xs, res, [&](const double* hx, size_t nxh, double* hr, size_t nrh) {
                         HK<E>::log_1d(hx, nxh, (unsigned)nxh, hr, nrh, (unsigned)nrh, seed);
                     }))
                K<E>::log_1d(R.stream, xs.p, xs.plane, (unsigned)xs.numel(), res.p, res.plane, (unsigned)res.numel(), seed);
            return;
        }
        log_rec(xs.index0(0), res.index0(0), seed);
        size_t n0 = res.shape[0];
        if (n0 <= 1) return;
        if (!host && recur_wavefront(WF_LOG, xs, xs, res)) return;
        // rs[j] = res[j] * j, filled slab by slab as res becomes known (mt:1362-1365)
        Rc<Buf> rsbuf = alloc_tier(host, res.numel() * W);
        HV rs{rsbuf->p, res.numel(), res.shape, host};
        zero_elems(host, rs.p, res.numel() * W);
        Dims sub(res.shape.begin() + 1, res.shape.end());
        HV x0 = xs.index0(0);
        // device tier: right-looking accumulation like div_rec — once rs[k] = res[k] * k is known, one product adds
        // xs[1..m] (*) rs[k] into the m slabs that follow (terms arrive in ascending j, as in the reference)
        const bool right = !host;
        Dims xrest(xs.shape.begin() + 1, xs.shape.end());
        if (right) {
            HV tail{res.p + prod(sub), res.plane, res.shape, false};
            zero_elems(false, tail.p, res.numel() - prod(sub));
            if (W == 2) zero_elems(false, tail.p + res.plane, res.numel() - prod(sub));
        }
        for (size_t k = 1; k < n0; ++k) {
            HV cur = res.index0(k);
            if (!right) conv(xs, rs, res, k, k + 1, false, true, 1, 1, 1);  // sum_{j} xs[k-j] (*) (res[j]*j), j ascending
            HV rk = rs.index0(k);
            bool step_done = false;
            if (right && cur.shape.size() == 2 && x0.numel() > 1) {
                // the whole slab step in one launch (gft_div2d.hip, fused == 2): neg, += k * xs[k], the 2-d division by xs[0]
                // — what Div's dispatcher (mt:1194-1231) comes to for a divisor of more than one coefficient —, / k, and
                // rs[k] = res[k] * k; element for element the sequence below
                const bool have_x = k < xs.shape[0];
                HV xk = have_x ? xs.index0(k) : HV{nullptr, 0, Dims{0, 0}, false};
                step_done = K<E>::div_2d(R.stream, xk.p, xk.plane, have_x ? (unsigned)xk.shape[0] : 0u, have_x ? (unsigned)xk.shape[1] : 0u,
                                         have_x ? xk.shape[1] : 0, x0.p, x0.plane, (unsigned)x0.shape[0], (unsigned)x0.shape[1], cur.p,
                                         cur.plane, (unsigned)cur.shape[0], (unsigned)cur.shape[1], 2, (unsigned)k, rk.p, rk.plane);
            }
            if (!step_done) {
                x_map_inplace(cur, MAP_NEG, 0);
                if (k < xs.shape[0]) x_block_op(cur, xs.index0(k), BLK_ADD_U32_TIMES, (unsigned)k);
                // current = current / xs[0] as full TaylorPoly division with degrees = current.shape (mt:1376-1383)
                P num = make(sub, sub, host), den = make(x0.shape, sub, host);
                copy_planes(host, tp<E>(num, host), num.numel, cur.p, cur.plane, cur.numel());
                copy_planes(host, tp<E>(den, host), den.numel, x0.p, x0.plane, x0.numel());
                P q = div_same_tier(num, den, host);
                if (q.shape != sub) throw Error("log: internal shape mismatch after division");
                copy_planes(host, cur.p, cur.plane, tp<E>(q, host), q.numel, cur.numel());
                x_map_inplace(cur, MAP_DIV_U32, (unsigned)k);
                copy_planes(host, rk.p, rk.plane, cur.p, cur.plane, cur.numel());
                x_map_inplace(rk, MAP_MUL_U32, (unsigned)k);
            }
            if (right && k + 1 < n0 && xs.shape[0] >= 2) {
                const size_t m = std::min(n0 - 1 - k, xs.shape[0] - 1);
                Dims xsm{m}, ys1{1}, zsm{m};
                xsm.insert(xsm.end(), xrest.begin(), xrest.end());
                ys1.insert(ys1.end(), sub.begin(), sub.end());
                zsm.insert(zsm.end(), sub.begin(), sub.end());
                HV xm{xs.p + prod(xrest), xs.plane, xsm, false}, yk{rk.p, rs.plane, ys1, false},
                    zm{res.p + (k + 1) * prod(sub), res.plane, zsm, false};
                right_update(xm, yk, zm, m);
            }
        }
        if (right) join_side();
    }
    // Div's dispatcher (mt:1194-1231) for the slab division inside log.  tp<E>() serves a device caller whatever side
    // the quotient is on; a host caller needs it in host memory.
    static P div_same_tier(const P& num, const P& den, bool host) {
        P q = div(num, den);
        if (host && !on_host(q)) {  // cannot happen while the dispatch criterion is monotone in the shapes; stay correct anyway
            P h = make(q.shape, q.deg, true);
            HIP_OK(hipMemcpyAsync(hp<E>(h), dp<E>(q), sizeof(double) * q.numel * W, hipMemcpyDeviceToHost, R.stream));
            HIP_OK(hipStreamSynchronize(R.stream));
            return h;
        }
        return q;
    }
    static P log(const P& a) {
        Dims rs = explog_shape(a);
        const bool host = tier_host(prod(rs), a) && est_macs(a.shape, rs, rs) <= R.host_max_macs;
        P out = make(rs, a.deg, host);
        log_rec(view(a, host), view(out, host), seed_of(a, false));
        return seal(out);
    }

    static P pow(const P& a, uint32_t e) {  // mt:433-451
        double one[2] = {1.0, 1.0};
        if (e == 0) return scalar(one);
        if (e == 1) return a;
        P res = scalar(one);
        P base = a;
        while (e > 0) {
            if (e & 1) res = mul(res, base);
            base = mul(base, base);  // includes the reference's redundant final squaring
            e >>= 1;
        }
        return res;
    }

    // Device-resident factor tables for derivative / coefficient expansion / index scaling depend only on
    // (kind, n, len): computed once by k_factor_table (reference operation order) and reused.
    static Rc<Buf> cached_table(int table_op, size_t n, size_t len, bool host = false) {
        static std::map<std::tuple<int, size_t, size_t>, Rc<Buf>> caches[2];
        auto& cache = caches[host ? 1 : 0];
        auto key = std::make_tuple(table_op, n, len);
        auto it = cache.find(key);
        if (it != cache.end()) {
            use_buf(it->second.get());  // (a table another stream uploaded: ordered before this stream's next launch)
            return it->second;
        }
        if (cache.size() > 4096) cache.clear();
        Rc<Buf> tab = alloc_tier(host, len * W);
        if (host) HK<E>::factor_table(table_op, (unsigned)n, (unsigned)len, nullptr, 0, tab->p, len);
        else if (len * W <= 1920) {
            // a data-independent table is a serial chain (a running product): one GPU lane takes 8 us for 200 f64 factors
            // and 90 us for 200 interval ones, a host core well under a microsecond — same functor, same bits; the values
            // travel as kernel arguments (no pinned staging, stream-ordered)
            std::vector<double> h(len * W);
            HK<E>::factor_table(table_op, (unsigned)n, (unsigned)len, nullptr, 0, h.data(), len);
            upload_small(R.stream, tab->p, h.data(), len * W);
        } else
            K<E>::factor_table(R.stream, table_op, (unsigned)n, (unsigned)len, nullptr, 0, tab->p, len);
        cache[key] = tab;
        return tab;
    }

