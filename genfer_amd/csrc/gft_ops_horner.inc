// Part of struct Ops<E> (included inside its body by gft_api.hip): subst_var (mt:540-580): the Horner loops — exact, speculative with witnesses, proven, recorded.
// Split out of gft_api.hip in round 6 by concern; no behavioural change (the compiler sees the same token stream).

    // ---- subst_var (mt:540-580) -----------------------------------------------------------------------------------------
    static P subst_var(const P& a, size_t v, const P& subst) {
        if (v >= a.shape.size()) return a;
        Dims deg = min_degrees(a, subst);
        if (is_zero(subst)) return slab_range(a, v, 0, 1, deg);
        double c[2], m[2];
        size_t w = 0;
        ScanCtx sc_subst("subst_var.subst");
        // A 2-element tensor is linear by structure; if the host also knows its constant term (see gft_poly::c0_known)
        // the verdict needs no device scan.  m stays on the device (the power table reads it from there).
        bool have_lin = false, m_known = true;
        if (subst.buf && !subst.buf->host && !subst.buf->lin_state && subst.numel == 2 && subst.c0_known && val_is_zero(subst.c0)) {
            for (size_t ax = 0; ax < subst.shape.size(); ++ax)
                if (subst.shape[ax] == 2) w = ax;
            if (v == w) {
                c[0] = subst.c0[0];
                c[1] = subst.c0[1];
                have_lin = true;
                m_known = false;
            }
        }
        if (!have_lin) have_lin = extract_linear(subst, c, m, &w);
        if (have_lin) {
            if (v == w && val_is_zero(c)) {
                Dims lens = a.shape;
                for (size_t i = 0; i < lens.size(); ++i) lens[i] = std::min(lens[i], deg[i]);
                if (m_known && val_is_one(m)) return lead_block(a, lens, deg);  // powers of one: x * 1 == x, nothing to compute
                Dims sst = c_strides(subst.shape);
                Shifts shift(lens.size(), 0);
                if (m_known && gather_tier(a, lens)) {  // host tier: the running product m^k per element (mt:557-565)
                    const double mm[2] = {m[0], m[1]};
                    return gather(a, lens, deg, shift, a.shape, OP_MUL_POW, nullptr, (int)v, mm, 1, nullptr, 1);
                }
                if (m_known && can_defer(a, prod(lens)) && lens.size() <= a.shape.size()) {
                    // deferred: x * m^k along v as a chain stage reading the per-m device table (no launch here)
                    P r = deferred(a, lens, deg, 1);
                    push_stage(r, CH_MUL_TAB, nullptr, (int)v, pow_table(m, lens[v]));
                    return r;
                }
                if (m_known) {
                    // m is known on the host: the powers m^k — the reference's running product ((1*m)*m)*.. (mt:557-565), the
                    // same functor on the host, so the same bits — are formed here.  Up to HTAB_CAP of them travel BY VALUE
                    // with the gather (no table launch, no per-thread running product, no device mirror of a host-resident
                    // subst); longer tables are uploaded.
                    std::vector<double> pw(lens[v] * W);
                    typename E::V f = E::one();
                    const typename E::V mv = E::from(Scalar2{m[0], W == 2 ? m[1] : 0.0});
                    for (size_t k = 0; k < lens[v]; ++k) {
                        E::st(pw.data(), lens[v], k, f);
                        f = E::mul(f, mv);
                    }
                    if (lens[v] <= (W == 1 ? HTAB_CAP : HTAB_CAP / 2))
                        return gather(a, lens, deg, shift, a.shape, OP_MUL_HTAB, nullptr, (int)v, pw.data(), lens[v], nullptr, 0);
                    Rc<Buf> tabh = alloc_doubles(lens[v] * W);
                    upload_small(R.stream, tabh->p, pw.data(), lens[v] * W);
                    return gather(a, lens, deg, shift, a.shape, OP_MUL_TAB, nullptr, (int)v, tabh->p, lens[v], nullptr, 0);
                }
                if (lens[v] <= 256)  // short axis: every thread forms its own m^k (same running product), no table launch
                    return gather(a, lens, deg, shift, a.shape, OP_MUL_POW, nullptr, (int)v, dp<E>(subst) + sst[w], subst.numel, nullptr, 0);
                Rc<Buf> tab = alloc_doubles(lens[v] * W);
                K<E>::factor_table(R.stream, TAB_POW, 0, (unsigned)lens[v], dp<E>(subst) + sst[w], subst.numel, tab->p, lens[v]);
                return gather(a, lens, deg, shift, a.shape, OP_MUL_TAB, nullptr, (int)v, tab->p, lens[v], nullptr, 0);
            }
        }
        Dims cshape = a.shape;
        while (cshape.size() < deg.size()) cshape.push_back(1);
        P ca = with_meta_unchecked(a, cshape);
        // linear substitution known from the scan above (memoised on subst's buffer): fused Horner steps
        const bool lin_known = extract_linear(subst, c, m, &w) && w < deg.size() && deg[w] >= 2;
        P res;
        if (R.fuse_horner && cshape[v] <= WIT_SLOTS && horner_speculative(ca, v, subst, deg, lin_known, c, m, w, &res)) return res;
        return horner_exact(ca, v, subst, deg);
    }
    // One Horner coefficient: a[.., i, ..] clipped to deg (mt:571-576)
    static P horner_coeff(const P& ca, size_t v, size_t i, const Dims& deg) {
        Dims out = ca.shape;
        out[v] = 1;
        for (size_t ax = 0; ax < out.size(); ++ax) out[ax] = std::min(out[ax], deg[ax]);
        Shifts shift(out.size(), 0);
        shift[v] = (long long)i;
        return gather(ca, out, deg, shift, ca.shape);
    }
    // The reference's loop, operation for operation (mt:569-579): every product goes through Mul's dispatcher, which asks
    // on every step whether the accumulator is linear (a device scan + host round trip for device tensors, free on the
    // host tier).
    static P horner_exact(const P& ca, size_t v, const P& subst, const Dims& deg) {
        ScanCtx sc_he("subst_var.horner_exact");
        P res = zero_with(deg);
        for (size_t i = ca.shape[v]; i-- > 0;) res = addsub(mul(res, subst), horner_coeff(ca, v, i, deg), false);
        return res;
    }
    // The same loop without a host round trip per step.  The reference asks on every step whether the ACCUMULATOR is
    // linear (and then multiplies the other way round, which compacts its stored shape).  That is the case while the top
    // coefficient slabs are zero or scalar-like; once the accumulator has been seen non-linear it stays so short of an
    // exact cancellation.  So: reference steps (with the scan) until the first "not linear" verdict, then fused /
    // scan-free steps that SPECULATE "still not linear" — and prove it: every accumulator produced on the way is
    // checked on the device for a witness of non-linearity (a non-zero coefficient at an index with two non-zero
    // coordinates or a coordinate >= 2), one sticky word per step, and ONE verdict read-back at the end of the loop.
    // A step without a witness (exact cancellation, or a support on unit positions of two axes) makes the function
    // return false and the caller redoes the loop with horner_exact: the stored shapes are the reference's in every
    // case, the extra cost is one round trip per subst_var instead of one per step.
    // a device tensor copied into a host-tier tensor (the caller has decided that the host is the better machine for it)
    static P to_host_tier(const P& dev) {
        P h = make(dev.shape, dev.deg, true);
        HIP_OK(hipMemcpyAsync(hp<E>(h), dp<E>(dev), sizeof(double) * dev.numel * W, hipMemcpyDeviceToHost, R.stream));
        HIP_OK(hipStreamSynchronize(R.stream));
        return h;
    }
    static constexpr size_t WIT_SLOTS = 8192;
    static bool horner_speculative(const P& ca, size_t v, const P& subst, const Dims& deg, bool lin_known, const double c[2],
                                   const double m[2], size_t w, P* result) {
        ScanCtx sc_hs("subst_var.horner_speculative");
        P res = zero_with(deg);
        bool res_nonlinear_seen = false;
        unsigned slots = 0;  // speculated accumulators so far (sticky witness words R.d_wit[0 .. slots))
        // Interval tensors with a substitution whose constant term c is a non-zero finite interval: interval arithmetic
        // cannot cancel — a product of two non-zero intervals and a sum with a non-zero term are widened, never [0,0]
        // (interval.rs:126-190) — and every step's out[k] contains the term c * res[k], so a non-zero coefficient of the
        // accumulator stays non-zero at its position for the rest of the loop.  The witness the initial scan found
        // therefore persists: the speculation is PROVEN and needs no per-step witnesses and no verdict read-back.
        bool proven = false;
        if (W == 2) {
            double c0[2];
            bool have = false;
            if (lin_known) { c0[0] = c[0]; c0[1] = c[1]; have = true; }
            else if (on_host(subst) || subst.c0_known || (subst.numel == 1 && subst.cached)) { first_value(subst, c0); have = true; }
            proven = have && !val_is_zero(c0) && (c0[0] - c0[0] == 0.0) && (c0[1] - c0[1] == 0.0);
        }
#ifdef GFT_DIAG  // measurement-only builds (make EXTRA=-DGFT_DIAG): skipping the verdict makes the speculation unsound
        static const bool verify = [] {
            const char* e = getenv("GFT_HORNER_VERIFY");
            return e ? atoi(e) != 0 : true;
        }();
        if (!verify) proven = true;
#endif
        // Host phase for LINEAR streaks (round 4).  The top coefficient slabs of a tensor with triangular support hold a
        // coefficient or two each: the accumulator stays linear for several steps, and on the device every one of them is a
        // scan, a host round trip and four launches of a few elements (hmm `--bounds`: 11 918 of its 16 300 scans said
        // "linear").  After the first such verdict the accumulator and the next HBLK coefficient slabs are brought to the
        // host tier (one gather, two copies) and the steps run there — the same reference steps on the same functors, their
        // scans free — until the accumulator is no longer linear or outgrows the tier; then the device takes over again.
        constexpr size_t HBLK = 8;
        P ca_h;                       // host-tier copy of the slabs [ca_h_lo, ca_h_hi) of ca along v
        size_t ca_h_lo = 0, ca_h_hi = 0;
        auto fetch_block = [&](size_t i_top) {
            const size_t lo = i_top + 1 > HBLK ? i_top + 1 - HBLK : 0;
            ca_h = to_host_tier(slab_range(ca, v, lo, i_top + 1, ca.deg, OP_COPY, -1, nullptr, 0, 0));
            ca_h_lo = lo;
            ca_h_hi = i_top + 1;
        };
        // (round 6) a proven loop on a tensor nothing is known about: ask once where its zeros are (nz_query: one launch and round
        // trip, what a single linearity scan costs — and the answer is inherited by everything computed from the tensor)
        if (W == 2 && proven && R.nz_proofs && !on_host(ca) && ca.numel >= 64 && ca.buf->nz == 0) {
            if (!ca.pend) (void)nz_query(ca);
            else if (!ca.pend->mat) {  // a chain: the question goes to its base tensor, the chain's stages carry the answer over
                P base;
                base.width = W;
                base.shape = ca.pend->base_shape;
                base.deg = ca.pend->base_shape;
                base.numel = ca.pend->base_numel;
                base.buf = ca.buf;
                if (base.numel >= 64 && prod(base.shape) == base.numel) (void)nz_query(base);
            }
        }
        for (size_t i = ca.shape[v]; i-- > 0;) {
            bool speculate = false;
            if (!on_host(res) && res.numel > 1) {
                // (round 5, intervals) a proven loop whose coefficient tensor holds no exact zero: the accumulator — a slab of it,
                // at least 3 coefficients — cannot be linear (nz_of_poly): no scan, no round trip; the verdict is memoised as
                // if the scan had delivered it
                if (!res_nonlinear_seen && W == 2 && proven && R.nz_proofs && res.numel >= 3 && res.buf &&
                    (nz_of(res) == 2 || (res.buf.get() == ca.buf.get() && nz_of(ca) == 0 && nz_query(ca) == 2 && nz_of(res) == 2) ||
                     support_proves_nonlinear(support_of_poly<E>(res), res.shape))) {
                    // (the loop reads the slab in place where it is a pure view — res_is_view —, from memory otherwise: dp() in
                    // launch_horner materialises it then)
                    if (!res.pend && res.buf && !res.buf->host && !res.buf->lin_state) res.buf->lin_state = 1;
                    res_nonlinear_seen = true;
                    R.stats_nz++;
                }
                if (!res_nonlinear_seen) {  // device accumulator: scan until the first "not linear" verdict
                    double c_[2], m_[2];
                    size_t u_;
                    ScanCtx sc_res("subst_var.accumulator");
                    const Support sr_pre = g_scan_trace.on ? support_of_poly<E>(res) : Support();
                    const int res_nz_pre = res.buf ? (int)res.buf->nz : -1, res_pend_pre = res.pend ? res.pend->n + 100 * (res.pend->base_off != 0) : -1;
                    const bool res_same_pre = res.buf.get() == ca.buf.get();
                    const bool res_lazy_pre = res.buf && res.buf->lazy != nullptr;
                    ScanToken tok = extract_linear_begin(res);
                    if (g_scan_trace.on && W == 2) {  // why no proof: what is known about the operand's and the accumulator's zeros
                        char key[200];
                        const Support sc = support_of_poly<E>(ca), sr = support_of_poly<E>(res);
                        std::string st;
                        if (ca.pend) {
                            st = ca.pend->padded ? "pad " : "";
                            for (int q = 0; q < ca.pend->n; ++q) st += std::to_string(ca.pend->st[q].kind) + ",";
                            if (ca.pend->base_off) st += "off";
                        }
                        (void)sr;
                        snprintf(key, sizeof key, "no proof: ca buf.nz=%d kind=%d pend=[%s] from %s | res BEFORE the scan: kind=%d buf.nz=%d pend=%d same_buf=%d lazy=%d numel=%s res_seen=%d",
                                 ca.buf ? (int)ca.buf->nz : -1, sc.kind, st.c_str(), ca.buf && ca.buf->origin ? ca.buf->origin : "?", sr_pre.kind, res_nz_pre, res_pend_pre, (int)res_same_pre,
                                 (int)res_lazy_pre, res.numel < 64 ? "<64" : ">=64", (int)res_nonlinear_seen);
                        g_scan_trace.counts[key]++;
                    }
                    if (g_scan_trace.on) {
                        char key[160];
                        snprintf(key, sizeof key, "horner scan: done=%d lin_known=%d rank_ok=%d i=%s proven=%d len_v=%s", (int)tok.done, (int)lin_known,
                                 (int)(res.shape.size() == deg.size()), i == 0 ? "0" : (i == 1 ? "1" : ">1"), (int)proven, ca.shape[v] == 2 ? "2" : ">2");
                        g_scan_trace.counts[key]++;
                    }
                    // The scan is in flight (or answered).  With a linear substitution the steps that follow a "not linear"
                    // verdict are ONE launch (horner_linear_rest): queue it right behind the scan, guarded on the device by
                    // the scan's verdict word, and only then wait for the verdict — the loop runs while the host reads its
                    // mail instead of after a launch latency on top of the round trip (`--bounds` programs: one scan per
                    // subst_var, 16-18 thousand of them).  A "linear" verdict (rare: the reference then multiplies the other
                    // way round) makes the queued launch a no-op; its output is dropped and the reference step is taken.
                    P ahead;
                    bool queued = false;
                    unsigned* ahead_wit = (proven || slots + (unsigned)i > WIT_SLOTS) ? nullptr : R.d_wit + slots;
                    bool queued_step = false;
                    if (!tok.done && R.fuse_horner && lin_known && res.shape.size() == deg.size()) {
                        if (i >= 1 && (proven || ahead_wit)) {
                            if (slots == 0 && !proven) HIP_OK(hipMemsetAsync(R.d_wit, 0, sizeof(unsigned) * WIT_SLOTS, R.stream));
                            // a proven loop on an operand the main chain has long passed: RECORDED (its launch needs no guard —
                            // nobody looks at the handle before the verdict below is in — and is dropped if the verdict is "linear")
                            queued = horner_linear_rest(res, ca, v, i, c, m, w, deg, &ahead, ahead_wit, R.d_flag + 16, proven && R.lazy_horner && R.batch_dag);
                        }
                        // ... or the single fused step where the whole-loop launch does not apply: the last step (nothing is
                        // speculated about its result), or any step of a proven loop (no witness to raise)
                        if (!queued && (i == 0 || proven)) {
                            ahead = horner_linear_step(res, ca, v, i, c, m, w, deg, R.d_flag + 16);
                            queued_step = true;
                        }
                    }
                    if (!extract_linear_end(tok, c_, m_, &u_)) res_nonlinear_seen = true;  // memoised: the generic mul reuses it
                    if (g_scan_trace.on) g_scan_trace.counts[res_nonlinear_seen ? "horner scan verdict: not linear" : "horner scan verdict: LINEAR"]++;
                    if (queued && res_nonlinear_seen) {
                        res = ahead;
                        if (!proven) slots += (unsigned)i;
                        break;
                    }
                    if (queued_step && res_nonlinear_seen) {
                        res = ahead;
                        if (i == 0) break;
                        continue;
                    }
                    // (queued and linear: `ahead` is dropped — its launch returned at the guard)
                    if (!res_nonlinear_seen && R.host_max_elems && res.numel <= R.host_max_elems && !on_host(ca) &&
                        prod(ca.shape) / ca.shape[v] * HBLK <= 16 * R.host_max_elems) {
                        res = to_host_tier(res);
                        fetch_block(i);
                        ++i;  // this step is taken again, on the host tier
                        continue;
                    }
                }
                speculate = res_nonlinear_seen;
            }
            if (!speculate) {  // reference step; on the host tier the accumulator's scan is free
                // Host-resident accumulator that is not linear, linear substitution: the step as ONE pass of the host tier
                // (gft_host.hpp horner_linear: the element order of mul -> mul_linear -> add -> add, no intermediate
                // tensors) — `--bounds` programs live on this path because subst - constant_term(subst) keeps a widened
                // constant.  Linearity is re-checked on every step (a host scan), so the stored shapes are the reference's.
                // (a host accumulator of a DEVICE tensor: the host phase above — its slabs come from the fetched block)
                const bool in_block = on_host(res) && !on_host(ca) && ca_h_hi > ca_h_lo;
                if (in_block && i < ca_h_lo) fetch_block(i);  // the streak outlasted the block
                if (in_block) {
                    double c_[2], m_[2];
                    size_t u_;
                    // (a PROVEN loop's device steps need not ask again; an unproven one scans the accumulator that arrives on the
                    // device — this verdict is about the accumulator BEFORE the step, and only witnesses cover results of steps)
                    if (res.numel > 1 && !extract_linear(res, c_, m_, &u_) && proven) res_nonlinear_seen = true;
                    res = addsub(mul(res, subst), horner_coeff(ca_h, v, i - ca_h_lo, deg), false);
                    continue;
                }
                if (lin_known && on_host(res) && on_host(ca) && res.numel > 1 && res.shape.size() == deg.size()) {
                    double c_[2], m_[2];
                    size_t u_;
                    if (!extract_linear(res, c_, m_, &u_)) {
                        // (the host scan's verdict carries over when the accumulator outgrows the host tier ONLY for a proven loop
                        // — it stays non-linear.  Otherwise the accumulator this step hands to the device is scanned there once:
                        // the witnesses of the speculative steps cover their own results, not the one they start from)
                        if (proven) res_nonlinear_seen = true;
                        // proven (interval, non-zero finite constant): the accumulator stays non-linear for the rest of the
                        // loop, so every remaining step runs in one host loop — two ping-pong buffers, no per-step scan,
                        // handle or shape vectors (they cost as much as the arithmetic on ~100-element tensors)
                        if (proven && horner_linear_rest_host(res, ca, v, i, c, m, w, deg, &res)) break;
                        res = horner_linear_step(res, ca, v, i, c, m, w, deg);
                        continue;
                    }
                }
                if (g_scan_trace.on && W == 2 && !on_host(ca)) {
                    P hc = horner_coeff(ca, v, i, deg);
                    P pr = mul(res, subst);
                    P nx = addsub(pr, hc, false);
                    char key[200];
                    snprintf(key, sizeof key, "reference step: coeff pend=%d off=%d same=%d | prod numel=%zu cached=%d host=%d | next pend=%d same=%d host=%d numel=%s", hc.pend ? hc.pend->n : -1,
                             hc.pend ? (int)(hc.pend->base_off != 0) : -1, (int)(hc.buf.get() == ca.buf.get()), pr.numel, (int)pr.cached, (int)on_host(pr), nx.pend ? nx.pend->n : -1,
                             (int)(nx.buf.get() == ca.buf.get()), (int)on_host(nx), nx.numel < 64 ? "<64" : ">=64");
                    g_scan_trace.counts[key]++;
                    res = nx;
                    continue;
                }
                res = addsub(mul(res, subst), horner_coeff(ca, v, i, deg), false);
                continue;
            }
            if (slots == 0 && !proven) HIP_OK(hipMemsetAsync(R.d_wit, 0, sizeof(unsigned) * WIT_SLOTS, R.stream));
            bool witnessed = false;
            if (lin_known && res.shape.size() == deg.size()) {
                // every remaining step in one launch (one workgroup per line along w); witnesses are raised in the kernel
                if (i >= 1 && horner_linear_rest(res, ca, v, i, c, m, w, deg, &res, proven ? nullptr : R.d_wit + slots, nullptr, proven && R.lazy_horner && R.batch_dag)) {
                    if (!proven) slots += (unsigned)i;  // the accumulators after the in-kernel steps 0 .. i-1 (the last one is the result)
                    break;
                }
                res = horner_linear_step(res, ca, v, i, c, m, w, deg);
            } else {
                P nxt;
                if (horner_general_step_fused(res, subst, ca, v, i, deg, (i > 0 && !proven) ? R.d_wit + slots : nullptr, &nxt)) {
                    res = nxt;
                    witnessed = true;  // (the step's kernel raised the witness word itself)
                } else {
                    res = addsub(mul_horner(res, subst), horner_coeff(ca, v, i, deg), false);
                }
            }
            if (on_host(res) || res.numel == 1) return false;  // left the speculated regime: take the exact loop
            if (i == 0) break;  // the last accumulator is the result: nothing is speculated about it
            if (!proven) {
                if (!witnessed) {
                    Dims keep = collapse_mask({&res.shape}, false);
                    HV rv = view(res);
                    K<E>::witness(R.stream, dview(rv, &keep), R.d_wit + slots);
                }
                slots++;
            }
        }
        if (slots) {
            Mailbox mb = next_mail();
            witness_verdict(R.stream, R.d_wit, slots, mb);
            R.stats[0]++;
            double missing = 0.0;
            wait_mail(mb, &missing, 1);
            if (missing != 0.0) return false;
        }
        if (g_scan_trace.on && W == 2 && res.buf && !res.buf->host) {
            char key[160];
            const Support sr = support_of_poly<E>(res), sc = support_of_poly<E>(ca);
            snprintf(key, sizeof key, "subst_var (speculative) result: kind=%d from ca kind=%d lin_known=%d proven=%d", sr.kind, sc.kind, (int)lin_known, (int)proven);
            g_scan_trace.counts[key]++;
        }
        *result = res;
        return true;
    }
    // res * subst inside the Horner loop once the accumulator has been seen non-linear.  The generic mul would ask
    // again on every step whether `res` is linear (device scan + host round trip, because res is new each time)
    // before it looks at `subst`, whose verdict is memoised; here only subst's verdict is consulted, and the
    // speculation "res is not linear" is verified by horner_speculative's witnesses.
    static P mul_horner(const P& res, const P& subst) {
        if (res.numel == 1 || subst.numel == 1) return mul(res, subst);
        P self = res, other = subst;
        Dims deg = min_degrees(self, other);
        broadcast(self, other);
        Dims shape = sum_shape(self, other);
        self = truncate_degrees(self, deg);
        other = truncate_degrees(other, deg);
        if (self.numel == 1 || other.numel == 1) return mul(res, subst);
        double c[2], m[2];
        size_t v;
        if (extract_linear(other, c, m, &v)) {
            Dims sh = self.shape;
            sh[v] = std::min(deg[v], sh[v] + 1);
            return mul_linear(self, c, m, v, sh, deg);
        }
        P out = make(shape, deg);
        conv(view(self), view(other), view(out), 0, shape.empty() ? 1 : shape[0], false, false, 0, 0, 0);
        return out;
    }
    // One GENERAL Horner step  res * subst + a[.., i, ..]  (mt:569-579) in ONE launch when the product is shallow (`subst`
    // a stencil of a few coefficients — the compound-distribution substitutions of Genfer's programs): the product's
    // reference-order sums, then Add's operations on each finished sum ((0 + prod) + slab, or element 0 += slab for a
    // 1-element slab), then the witness of non-linearity the speculative loop needs — instead of product (+ prep / reduce /
    // guard launches on the tiled kernel) + slab gather + add + witness.  Operation for operation what
    // addsub(mul_horner(res, subst), horner_coeff(ca, v, i, deg)) computes (the product on the reference-order kernel), so
    // the result carries the reference's bits.  false: not this case — nothing launched, the caller takes that sequence.
    static bool horner_general_step_fused(const P& res, const P& subst, const P& ca, size_t v, size_t i, const Dims& deg,
                                          unsigned* wit, P* result) {
        if (!R.shallow_max_terms || R.conv_mode != 0) return false;
        if (res.numel == 1 || subst.numel == 1 || on_host(res)) return false;
        P self = res, other = subst;
        Dims mdeg = min_degrees(self, other);
        broadcast(self, other);
        Dims shape = sum_shape(self, other);
        const size_t nd = shape.size();
        if (nd != deg.size() || ca.shape.size() != nd) return false;
        for (size_t ax = 0; ax < nd; ++ax)  // nothing to truncate (the loop's accumulators never exceed deg)
            if (self.shape[ax] > mdeg[ax] || other.shape[ax] > mdeg[ax]) return false;
        size_t terms = 1;
        for (size_t ax = 0; ax < nd; ++ax) terms *= std::min(self.shape[ax], other.shape[ax]);
        if (terms > R.shallow_max_terms) return false;
        {
            double c[2], m[2];
            size_t u;
            if (extract_linear(other, c, m, &u)) return false;  // (memoised on subst's buffer) the mul_linear path is the reference's
        }
        // the Add: degrees, the slab's box, the result's shape (mt:854-882)
        Dims rd(nd, UMAX), oc = ca.shape;
        oc[v] = 1;
        for (size_t ax = 0; ax < nd; ++ax) {
            rd[ax] = std::min(mdeg[ax], deg[ax]);
            oc[ax] = std::min(oc[ax], deg[ax]);
            if (shape[ax] > rd[ax] || oc[ax] > rd[ax]) return false;
        }
        const bool slab_scalar = prod(oc) == 1;
        Dims oshape = shape;
        if (!slab_scalar)
            for (size_t ax = 0; ax < nd; ++ax) oshape[ax] = std::max(shape[ax], oc[ax]);
        // the kernel's loop nest is the reference's only if the product's own non-unit axes are the output's
        for (size_t ax = 0; ax < nd; ++ax)
            if ((oshape[ax] > 1) != (shape[ax] > 1)) return false;
        Dims keep = collapse_mask({&shape}, false);
        if (keep.empty() || keep.size() > 6) return false;
        ConvArgs a;
        std::memset(&a, 0, sizeof(a));
        ConvEpi e;
        std::memset(&e, 0, sizeof(e));
        a.nd = (int)keep.size();
        Dims xs = pick(self.shape, keep), ys = pick(other.shape, keep), zs = pick(shape, keep);
        Dims xst = c_strides(xs), yst = c_strides(ys), zst = c_strides(zs), cst = c_strides(ca.shape);
        for (int j = 0; j < a.nd; ++j) {
            a.xs[j] = (unsigned)xs[j];
            a.ys[j] = (unsigned)ys[j];
            a.zs[j] = (unsigned)zs[j];
            a.xstr[j] = xst[j];
            a.ystr[j] = yst[j];
            a.zstr[j] = zst[j];
            e.os[j] = (unsigned)oshape[keep[j]];
            e.abox[j] = (unsigned)oc[keep[j]];
            e.astr[j] = keep[j] == v ? 0 : cst[keep[j]];
        }
        a.slab_lo = 0;
        a.slab_hi = a.zs[0];
        a.inner_from_zero = 1;  // every kept axis is non-unit: the last one is the reference's 1-d base case (mt:992-1000)
        a.variant = R.conv_variant;
        e.mode = slab_scalar ? 2 : 1;
        const double* cap = dp<E>(ca);  // (a deferred / host-tier coefficient tensor is materialised once for the whole loop)
        e.ap = cap + i * cst[v];
        e.aplane = ca.numel;
        e.wit = wit;
        const double* xp_ = dp<E>(self);
        const double* yp_ = dp<E>(other);
        P out = make(oshape, rd);
        if (!K<E>::conv_shallow(R.stream, xp_, self.numel, yp_, other.numel, out.buf->p, out.numel, a, e)) return false;
        R.stats[5]++;
        R.stats_shallow[0]++;
        R.stats_shallow[1]++;
        *result = out;
        return true;
    }
    // res * (c + m*eps_w) + a[.., i, ..] in one launch (k_horner_linear), element for element the sequence
    // mul -> mul_linear -> mul_var / scale / add -> add that the generic loop above performs.  The generic mul
    // would first ask whether `res` itself is linear (a device scan + host round trip per step) and, if so,
    // multiply the other way round; these kernels speculate that it is not and raise a witness per step
    // (horner_speculative), so a step where the speculation fails is redone by the exact loop.
    // Steps i, i-1, .., 0 in one launch (k_horner_linear_loop) when the final tensor is small enough for a single
    // workgroup to be the faster machine (a launch per step costs ~4 us of host time + ~4 us on the device).
    // The first accumulator of a Horner loop is the top coefficient slab: a sub-box VIEW of the coefficient tensor with the
    // stage "element 0 + [0,0]" from the reference's first step (0 * subst + slab).  For intervals that stage returns its
    // operand unchanged unless the operand is itself zero (iv:126-134), so where the tensor is proven free of exact zeros the
    // view IS the sub-box, bit for bit, and the loop kernel reads it in place (base pointer + the tensor's strides) instead of
    // from a materialised copy — one launch less per subst_var.
    static bool res_is_view(const P& res, const P& ca) {
        if (W != 2 || !R.nz_proofs || !res.pend || !res.buf || res.buf.get() != ca.buf.get() || ca.pend || res.buf->host) return false;
        const Pend& q = *res.pend;
        if (q.padded || q.mat || q.base_shape.size() != res.shape.size() || !(q.base_shape == ca.shape)) return false;
        for (int i = 0; i < q.n; ++i) {
            const PendStage& g = q.st[i];
            if (!((g.kind == CH_FIRST_ADD || g.kind == CH_FIRST_SUB) && g.s[0] == 0.0 && g.s[1] == 0.0)) return false;
        }
        return nz_of(res) == 2;
    }
    // A recorded linear Horner loop (horner_linear_rest with `defer`): everything its launch needs.
    struct LazyHorner {
        P res, ca;                  // incoming accumulator and coefficient tensor (keep their buffers alive)
        HornerLoopArgs g;
        unsigned lines = 0;
        size_t fn = 0;
    };
    // Launches a loop — a recorded one into its own buffer, or a fresh one (the unbatched form; a recording with "batch_dag" on is
    // issued with its level of the launch graph, gft_api_dag.inc HornerRec).
    static void launch_horner(const P& res, const P& ca, double* outp, size_t fn, const HornerLoopArgs& g, unsigned lines, unsigned* wit) {
        const double* cp = dp<E>(ca);
        const bool rview = res_is_view(res, ca);  // (as when the arguments were built: the handle keeps its own chain)
        const double* rp = rview ? cp + res.pend->base_off : dp<E>(res);
        const size_t rplane = rview ? res.pend->base_numel : res.numel;
        K<E>::horner_linear_loop(R.stream, rp, rplane, cp, ca.numel, outp, fn, g, lines, wit);
    }
    static bool horner_linear_rest(const P& res, const P& ca, size_t v, size_t i, const double c[2], const double m[2], size_t w,
                                   const Dims& deg, P* result, unsigned* wit, const unsigned* guard = nullptr, bool defer = false) {
        const size_t nd = deg.size();
        Dims oc = ca.shape;
        oc[v] = 1;
        for (size_t ax = 0; ax < nd; ++ax) oc[ax] = std::min(oc[ax], deg[ax]);
        const bool coeff_scalar = prod(oc) == 1;
        Dims fs = res.shape;  // shape after all remaining steps
        for (size_t t = 0; t <= i; ++t) {
            fs[w] = std::min(deg[w], fs[w] + 1);
            if (!coeff_scalar)
                for (size_t ax = 0; ax < nd; ++ax) fs[ax] = std::max(fs[ax], oc[ax]);
        }
        const size_t fn = prod(fs);
        if (fn > R.horner_loop_max || fs[w] > K<E>::HORNER_LINE_MAX || fn / fs[w] > 0x7fffffffu) return false;
        Dims keep = collapse_mask({&fs}, false);
        if (keep.size() > (size_t)MAXD) return false;
        P out = make_recorded(fs, deg);  // (memory when the loop is launched: here below, or with its level of the launch graph)
        HornerLoopArgs g;
        std::memset(&g, 0, sizeof(g));
        g.nd = (int)keep.size();
        const bool rview = res_is_view(res, ca);
        Dims rst = c_strides(rview ? res.pend->base_shape : res.shape), fst = c_strides(fs), ast = c_strides(ca.shape);
        g.w = -1;
        for (size_t j = 0; j < keep.size(); ++j) {
            size_t ax = keep[j];
            g.deg[j] = (unsigned)std::min<size_t>(deg[ax], 0x7fffffffu);
            g.rs0[j] = (unsigned)res.shape[ax];
            g.fs[j] = (unsigned)fs[ax];
            g.oc[j] = (unsigned)oc[ax];
            g.rstr0[j] = rst[ax];
            g.fstr[j] = fst[ax];
            g.astr[j] = ax == v ? 0 : ast[ax];
            if (ax == w) g.w = (int)j;
        }
        if (g.w < 0) return false;
        g.a_vstride = ast[v];
        g.first_i = (unsigned)i;
        g.nsteps = (unsigned)(i + 1);
        g.c = Scalar2{c[0], W == 2 ? c[1] : 0.0};
        g.m = Scalar2{m[0], W == 2 ? m[1] : 0.0};
        g.c_zero = val_is_zero(c) ? 1 : 0;
        g.c_one = val_is_one(c) ? 1 : 0;
        g.coeff_scalar = coeff_scalar ? 1 : 0;
        g.lw_pad = (unsigned)((fs[w] + 7) / 8 * 8);
        g.diag = 0;
        g.stat = nullptr;
        g.guard = guard;
        // (intervals, c and m not [0,0]) no exact zero among the coefficients, none in the result: position (o, k_w) of the final
        // box receives coeff_i[o, k'] * C(i,j) c^(i-j) m^j for every k' + j = k_w — at least one such term exists, none cancels
        if (W == 2) {
            // (round 6, Support) leading zero slabs on the other axes stay where they are; along the substituted axis every
            // position receives a term from the top coefficient slab
            Support sp = support_of_poly<E>(ca);
            if (sp.exact() && scale_keeps_zero_pattern(c) && scale_keeps_zero_pattern(m)) {  // (a zero slab times an infinite bound is NaN)
                if (v < (size_t)Buf::ZAX) sp.z[v] = 0;
                sp.kind = 3;
                sp.normalise();
            } else
                sp.kind = 0;
            sp.store(out.buf.get());
        }
        const unsigned lines = (unsigned)(fn / fs[w]);
        if (defer && !wit && res.buf && ca.buf) {
            g.guard = nullptr;
            if (K<E>::horner_can_ride(g)) {
                auto lh = rc_allocate<LazyHorner>(gft_small::Alloc<LazyHorner>());
                // (measured and not kept: the loop's chain operands as recorded materialisations, SettleRec as for observation chains —
                // hmm --bounds forces a graph every few recordings, the 1 940 extra nodes batched 112 launches away and cost 0.247 -> 0.285 s)
                lh->res = res;
                lh->ca = ca;
                lh->g = g;
                lh->lines = lines;
                lh->fn = fn;
                auto op = rc_allocate<LazyOp>(gft_small::Alloc<LazyOp>());
                op->horner = lh;
                op->run = [lh](Buf* b) { launch_horner(lh->res, lh->ca, b->p, lh->fn, lh->g, lh->lines, nullptr); };
                auto rec = rc_allocate<HornerRec>(gft_small::Alloc<HornerRec>());
                rec->lh = lh;
                op->rec = rec;
                out.buf->lazy = op;
                *result = out;
                return true;
            }
            g.guard = guard;
        }
        ensure_alloc(out.buf.get());
        launch_horner(res, ca, dp<E>(out), fn, g, lines, wit);
        *result = out;
        return true;
    }
    // Steps i0, i0-1, .., 0 of the linear Horner loop on HOST-resident operands, one pass of HK::horner_linear per step
    // (exactly horner_linear_step's arguments, unit axes kept instead of collapsed), without the per-step handles.
    static bool horner_linear_rest_host(const P& res0, const P& ca, size_t v, size_t i0, const double c[2], const double m[2],
                                        size_t w, const Dims& deg, P* result) {
        const size_t nd = deg.size();
        if (nd == 0 || nd > (size_t)MAXD || res0.shape.size() != nd || ca.shape.size() != nd) return false;
        Dims oc = ca.shape;
        oc[v] = 1;
        for (size_t ax = 0; ax < nd; ++ax) oc[ax] = std::min(oc[ax], deg[ax]);
        const bool coeff_scalar = prod(oc) == 1;
        auto step_shapes = [&](const Dims& rs, Dims& sh, Dims& os) {
            sh = rs;
            sh[w] = std::min(deg[w], sh[w] + 1);
            os = sh;
            if (!coeff_scalar)
                for (size_t ax = 0; ax < nd; ++ax) os[ax] = std::min(std::max(sh[ax], oc[ax]), deg[ax]);
        };
        Dims rs = res0.shape, sh, os, fs = res0.shape;
        size_t cap = 0;
        for (size_t t = 0; t <= i0; ++t) {  // largest intermediate (shapes only grow)
            step_shapes(fs, sh, os);
            fs = os;
            cap = std::max(cap, prod(os));
        }
        if (!tier_host(cap, res0, ca)) return false;
        P out = make(fs, deg, true);
        Rc<Buf> ping = alloc_host_doubles(cap * W), pong = alloc_host_doubles(cap * W);
        const double* src = hp<E>(res0);
        size_t src_plane = res0.numel;
        const Dims ast = c_strides(ca.shape);
        HornerArgs g;
        std::memset(&g, 0, sizeof(g));
        g.c = Scalar2{c[0], W == 2 ? c[1] : 0.0};
        g.m = Scalar2{m[0], W == 2 ? m[1] : 0.0};
        g.c_zero = val_is_zero(c) ? 1 : 0;
        g.c_one = val_is_one(c) ? 1 : 0;
        g.coeff_scalar = coeff_scalar ? 1 : 0;
        g.w = (int)w;
        g.out.nd = (int)nd;
        for (size_t ax = 0; ax < nd; ++ax) {
            g.oc[ax] = (unsigned)oc[ax];
            g.astr[ax] = ax == v ? 0 : ast[ax];
        }
        for (size_t i = i0, t = 0;; --i, ++t) {
            step_shapes(rs, sh, os);
            size_t stride = 1;
            for (size_t ax = nd; ax-- > 0;) {
                g.out.d[ax] = (unsigned)os[ax];
                g.rs[ax] = (unsigned)rs[ax];
                g.sh[ax] = (unsigned)sh[ax];
                g.rstr[ax] = stride;
                stride *= rs[ax];
            }
            g.a_base = i * ast[v];
            g.upper = (unsigned)std::min(sh[w] - 1, rs[w]);
            const size_t n_out = prod(os);
            double* dst = i == 0 ? hp<E>(out) : ((t & 1) ? pong->p : ping->p);
            HK<E>::horner_linear(src, src_plane, hp<E>(ca), ca.numel, dst, n_out, g);
            rs = os;
            src = dst;
            src_plane = n_out;
            if (i == 0) break;
        }
        *result = seal(out);
        return true;
    }
    static P horner_linear_step(const P& res, const P& ca, size_t v, size_t i, const double c[2], const double m[2], size_t w,
                                const Dims& deg, const unsigned* guard = nullptr) {
        const size_t nd = deg.size();
        Dims rs = res.shape, sh = res.shape, oc = ca.shape;
        sh[w] = std::min(deg[w], sh[w] + 1);
        oc[v] = 1;
        for (size_t ax = 0; ax < nd; ++ax) oc[ax] = std::min(oc[ax], deg[ax]);
        const bool coeff_scalar = prod(oc) == 1;
        Dims os = sh;
        if (!coeff_scalar)
            for (size_t ax = 0; ax < nd; ++ax) os[ax] = std::min(std::max(sh[ax], oc[ax]), deg[ax]);
        const bool host = tier_host(prod(os), res, ca);
        P out = make(os, deg, host);
        Dims keep = collapse_mask({&os}, false);
        if (keep.size() > (size_t)MAXD) throw Error("tensor rank exceeds GFT MAXD after collapsing");
        HornerArgs g;
        std::memset(&g, 0, sizeof(g));
        g.out = to_shape(pick(os, keep));
        Dims rst = c_strides(rs), ast = c_strides(ca.shape);
        g.w = -1;
        for (size_t j = 0; j < keep.size(); ++j) {
            size_t ax = keep[j];
            g.rs[j] = (unsigned)rs[ax];
            g.sh[j] = (unsigned)sh[ax];
            g.oc[j] = (unsigned)oc[ax];
            g.rstr[j] = rst[ax];
            g.astr[j] = ax == v ? 0 : ast[ax];
            if (ax == w) g.w = (int)j;
        }
        if (g.w < 0) throw Error("horner_linear_step: substitution axis collapsed");  // sh[w] >= 2 => kept
        g.a_base = i * ast[v];
        g.upper = (unsigned)std::min(sh[w] - 1, rs[w]);
        g.c = Scalar2{c[0], W == 2 ? c[1] : 0.0};
        g.m = Scalar2{m[0], W == 2 ? m[1] : 0.0};
        g.c_zero = val_is_zero(c) ? 1 : 0;
        g.c_one = val_is_one(c) ? 1 : 0;
        g.coeff_scalar = coeff_scalar ? 1 : 0;
        if (host) {
            HK<E>::horner_linear(hp<E>(res), res.numel, hp<E>(ca), ca.numel, hp<E>(out), out.numel, g);
            return seal(out);
        }
        g.guard = guard;
        K<E>::horner_linear(R.stream, dp<E>(res), res.numel, dp<E>(ca), ca.numel, dp<E>(out), out.numel, g);
        return out;
    }
    static P with_meta_unchecked(const P& src, const Dims& shape) {
        P r = src;
        r.shape = shape;
        return r;
    }

