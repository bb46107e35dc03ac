// Part of struct Ops<E> (included inside its body by gft_api.hip): handles in the two tiers, allocation, deferred chains, value inspection, shape helpers, structured copies, constructors, Add / Sub / Neg, extract_linear.
// Split out of gft_api.hip in round 6 by concern; no behavioural change (the compiler sees the same token stream).

    // ---- size-threshold dispatch (SURVEY §8f-2) ------------------------------------------------------------
    // An operation runs on the host tier iff every operand is host-resident and its result is small.
    static bool tier_host(size_t out_numel, const P& a) {
        return R.host_max_elems && out_numel <= R.host_max_elems && on_host(a);
    }
    static bool tier_host(size_t out_numel, const P& a, const P& b) { return tier_host(out_numel, a) && on_host(b); }
    // 1-element results of the host tier become lazy scalars (value in the handle, no buffer at all)
    static P seal(P& r_) {  // (the caller's last use of its local: moved from, not copied)
        P r = std::move(r_);
        if (r.buf && r.buf->host) {
            R.stats[6]++;
            if (r.numel == 1) {
                r.cv[0] = r.buf->p[0];
                r.cv[1] = W == 2 ? r.buf->p[1] : 0.0;
                r.cached = true;
                r.lazy_lin = false;
                r.buf = nullptr;
            }
        }
        return r;
    }
    static V2 hv(const double v[2]) { return V2{v[0], W == 2 ? v[1] : 0.0}; }
    // device-to-device copies and memsets keep their place among the queued launches (gft_launch.hpp): they are queued
    // too instead of making the API thread wait for the launch thread
    static void copy_elems(bool host, double* dst, const double* src, size_t n) {
        if (host) std::memcpy(dst, src, sizeof(double) * n);
        else {
            hipStream_t st = R.stream;
            enqueue_task([=] { lq_note((hipMemcpyAsync)(dst, src, sizeof(double) * n, hipMemcpyDeviceToDevice, st), nullptr, "hipMemcpyAsync (device to device)"); });
        }
    }
    static void zero_elems(bool host, double* dst, size_t n) {
        if (host) std::memset(dst, 0, sizeof(double) * n);
        else {
            hipStream_t st = R.stream;
            enqueue_task([=] { lq_note((hipMemsetAsync)(dst, 0, sizeof(double) * n, st), nullptr, "hipMemsetAsync"); });
        }
    }
    static DView dview(const HV& v, const Dims* keep = nullptr) {
        DView d;
        d.p = v.p;
        d.plane = v.plane;
        d.sh = to_shape(keep ? pick(v.shape, *keep) : v.shape);
        return d;
    }

    // ---- allocation ------------------------------------------------------------------------
    static P make(const Dims& shape, const Dims& deg, bool host = false) {
        check_invariants(shape, deg);
        P r;
        r.width = W;
        r.shape = shape;
        r.deg = deg;
        r.numel = prod(shape);
        r.buf = alloc_tier(host, r.numel * W);
        return r;
    }
    // the result of a RECORDED operation: shape, degrees and every host-visible fact now, memory when it is launched
    static P make_recorded(const Dims& shape, const Dims& deg) {
        check_invariants(shape, deg);
        P r;
        r.width = W;
        r.shape = shape;
        r.deg = deg;
        r.numel = prod(shape);
        r.buf = alloc_recorded(r.numel * W);
        return r;
    }
    static P with_meta(const P& src, const Dims& shape, const Dims& deg) {  // metadata-only reshape
        check_invariants(shape, deg);
        P r = src;
        r.shape = shape;
        r.deg = deg;
        return r;
    }
    static P from_host_value(typename E::V v, const Dims& shape, const Dims& deg) {
        double x[2] = {0.0, 0.0};
        E::st(x, 1, 0, v);
        R.stats[6]++;
        return from_host_scalar(x, shape, deg);
    }
    static P from_host_scalar(const double* x, const Dims& shape, const Dims& deg) {
        check_invariants(shape, deg);
        P r;
        r.width = W;
        r.shape = shape;
        r.deg = deg;
        r.numel = 1;
        r.cached = true;   // lazy: no device buffer until a kernel has to read it (see dp())
        r.cv[0] = x[0];
        r.cv[1] = W == 2 ? x[1] : 0.0;
        return r;
    }
    static P copy_of(const P& a) {
        P r = make(a.shape, a.deg);
        HIP_OK(hipMemcpyAsync(dp<E>(r), dp<E>(a), sizeof(double) * a.numel * W, hipMemcpyDeviceToDevice, R.stream));
        return r;
    }

    // ---- deferred elementwise chains (gft_kernels.hpp ChainSrc; struct Pend above) ---------------------------------------
    // An elementwise operation on a device tensor is not launched: the result handle shares the operand's buffer and
    // records the operation; the kernel that eventually consumes it applies the recorded stages, in order, to every
    // element it loads (same functors => the bits of one launch per operation).  Tensors of fewer than 4 elements and
    // everything host-resident keep the direct paths.
    static ChainSrc chain_src_dev(const P& p, const Dims& keep) {
        ChainSrc c = chain_src<E>(p, keep);
        if (!p.pend) c.p = dp<E>(p);  // a host-tier tensor is read through its device mirror
        return c;
    }
    static bool can_defer(const P& src, size_t out_numel) {
        return R.defer && src.buf && !src.buf->host && out_numel >= 4;
    }
    // element 0 after one more stage, from element 0 before it (host side of a chain: same functors, same bits)
    static void stage_apply_first(const PendStage& g, double v[2]) {
        typename E::V x = E::from(hv(v));
        const typename E::V sv = E::from(hv(g.s));
        switch (g.kind) {
            case CH_LMUL_S: x = E::mul(sv, x); break;
            case CH_MUL_S: x = E::mul(x, sv); break;
            case CH_DIV_S: x = E::div(x, sv); break;
            case CH_NEG: x = E::neg(x); break;
            case CH_FIRST_ADD: x = E::add(x, sv); break;
            case CH_FIRST_SUB: x = E::sub(x, sv); break;
            case CH_FIRST_SUB_NEG_ALL: x = E::neg(E::sub(x, sv)); break;
            case CH_MUL_TAB: x = E::mul(x, E::ld(g.tab->host.data(), g.tab->len, 0)); break;
            default: break;
        }
        double o[2] = {0.0, 0.0};
        E::st(o, 1, 0, x);
        v[0] = o[0];
        v[1] = W == 2 ? o[1] : 0.0;
    }
    // `src` restricted to its leading box `out_shape`, with room for `extra` more stages: a handle that shares src's
    // base buffer and copies its chain.  (A chain that is full, or that somebody has already materialised, restarts
    // from the materialised tensor.)
    static P deferred(const P& src, const Dims& out_shape, const Dims& out_deg, int extra) {
        check_invariants(out_shape, out_deg);
        if (src.pend && (src.pend->n + extra > CHAIN_MAX || src.pend->mat || src.pend->padded)) settle<E>(src);
        P r;
        r.width = W;
        r.shape = out_shape;
        r.deg = out_deg;
        r.numel = prod(out_shape);
        r.buf = src.buf;
        r.c0_known = src.c0_known;
        r.c0[0] = src.c0[0];
        r.c0[1] = src.c0[1];
        r.pend = rc_allocate<Pend>(gft_small::Alloc<Pend>());
        if (src.pend) {
            r.pend->base_shape = src.pend->base_shape;
            r.pend->base_numel = src.pend->base_numel;
            r.pend->base_off = src.pend->base_off;
            r.pend->n = src.pend->n;
            for (int i = 0; i < src.pend->n; ++i) r.pend->st[i] = src.pend->st[i];
        } else {
            r.pend->base_shape = src.shape;
            r.pend->base_numel = src.numel;
        }
        return r;
    }
    static void push_stage(P& r, int kind, const double* sv, int axis = 0, Rc<TabEntry> tab = nullptr) {
        Pend& q = *r.pend;
        if (q.n >= CHAIN_MAX) throw Error("internal: deferred chain overflow");
        if (q.padded) throw Error("internal: stage after a pad");
        PendStage& g = q.st[q.n++];
        g.kind = kind;
        g.axis = axis;
        g.s[0] = sv ? sv[0] : 0.0;
        g.s[1] = (sv && W == 2) ? sv[1] : 0.0;
        g.tab = tab;
        if (r.c0_known) stage_apply_first(g, r.c0);
        R.stats_ex[0]++;
    }
    // powers m^k, k < len, of a scaling substitution: the reference's running product ((1*m)*m)*.. (mt:557-565) on the
    // host tier's functor, kept on the device per value of m (a longer request re-forms the table: the running product
    // makes every table a prefix of the longer one)
    static Rc<TabEntry> pow_table(const double m[2], size_t len) {
        // (file-scope registry, one per element width: gft_shutdown releases it with the pool it allocates from)
        std::map<std::tuple<unsigned long long, unsigned long long>, Rc<TabEntry>>& cache = g_pow_tabs[W - 1];
        unsigned long long k0, k1 = 0;
        std::memcpy(&k0, &m[0], 8);
        if (W == 2) std::memcpy(&k1, &m[1], 8);
        auto key = std::make_tuple(k0, k1);
        auto it = cache.find(key);
        if (it != cache.end() && it->second->len >= len) return it->second;
        if (cache.size() > 256) cache.clear();
        size_t want = std::max<size_t>(len, 64);
        if (it != cache.end()) want = std::max(want, 2 * it->second->len);
        auto t = rc_make<TabEntry>();
        t->len = want;
        t->host.resize(want * W);
        typename E::V f = E::one();
        const typename E::V mv = E::from(Scalar2{m[0], W == 2 ? m[1] : 0.0});
        for (size_t k = 0; k < want; ++k) {
            E::st(t->host.data(), want, k, f);
            f = E::mul(f, mv);
        }
        t->dev = alloc_doubles(want * W);
        upload_small(R.stream, t->dev->p, t->host.data(), want * W);
        cache[key] = t;
        return t;
    }

    // ---- value inspection (the only host syncs) ---------------------------------------------
    static void first_value(const P& p, double out[2]) {
        if ((p.numel == 1 && p.cached) || (!p.buf && p.lazy_lin)) {  // host-known element 0
            out[0] = p.cv[0];
            out[1] = p.cv[1];
            return;
        }
        if (p.c0_known) {
            out[0] = p.c0[0];
            out[1] = p.c0[1];
            return;
        }
        if (p.pend) {  // element 0 of the base, then the chain's stages on the host (same functors)
            double v[2] = {0, 0};
            R.stats[1]++;
            use_buf(p.buf.get());
            peek(v, p.buf->p + p.pend->base_off, p.pend->base_numel, W);
            for (int i = 0; i < p.pend->n; ++i) stage_apply_first(p.pend->st[i], v);
            out[0] = v[0];
            out[1] = v[1];
            p.c0_known = true;
            p.c0[0] = v[0];
            p.c0[1] = v[1];
            return;
        }
        if (p.buf && p.buf->host) {
            out[0] = p.buf->p[0];
            out[1] = W == 2 ? p.buf->p[p.numel] : 0.0;
            return;
        }
        double tmp[2] = {0, 0};
        R.stats[1]++;
        peek(tmp, dp<E>(p), p.numel, W);
        out[0] = tmp[0];
        out[1] = tmp[1];
        if (p.numel == 1) {
            p.cached = true;
            p.cv[0] = tmp[0];
            p.cv[1] = tmp[1];
        } else {
            p.c0_known = true;
            p.c0[0] = tmp[0];
            p.c0[1] = tmp[1];
        }
    }
    static bool val_is_zero(const double v[2]) { return W == 1 ? v[0] == 0.0 : (v[0] == 0.0 && v[1] == 0.0); }
    static bool val_is_one(const double v[2]) { return W == 1 ? v[0] == 1.0 : (v[0] == 1.0 && v[1] == 1.0); }
    static bool is_zero(const P& p) {  // mt:643-645
        if (p.numel != 1) return false;
        double v[2];
        first_value(p, v);
        return val_is_zero(v);
    }
    static bool is_one(const P& p) {  // mt:653-655
        if (p.numel != 1) return false;
        double v[2];
        first_value(p, v);
        return val_is_one(v);
    }

    // ---- shape helpers (mt:114-204, 832-852) ---------------------------------------------------
    static Dims min_degrees(const P& a, const P& b) {
        Dims d(std::max(a.deg.size(), b.deg.size()), UMAX);
        for (size_t v = 0; v < d.size(); ++v) {
            if (v < a.deg.size()) d[v] = std::min(d[v], a.deg[v]);
            if (v < b.deg.size()) d[v] = std::min(d[v], b.deg[v]);
        }
        return d;
    }
    static Dims max_shape(const P& a, const P& b) {
        Dims s(std::max(a.shape.size(), b.shape.size()), 1);
        for (size_t v = 0; v < s.size(); ++v) {
            if (v < a.shape.size()) s[v] = std::max(s[v], a.shape[v]);
            if (v < b.shape.size()) s[v] = std::max(s[v], b.shape[v]);
            if (v < a.deg.size()) s[v] = std::min(s[v], a.deg[v]);
            if (v < b.deg.size()) s[v] = std::min(s[v], b.deg[v]);
        }
        return s;
    }
    static Dims sum_shape(const P& a, const P& b) {
        Dims s(std::max(a.shape.size(), b.shape.size()), 0);
        for (size_t v = 0; v < s.size(); ++v) {
            if (v < a.shape.size()) s[v] += a.shape[v] - 1;
            if (v < b.shape.size()) s[v] += b.shape[v] - 1;
            s[v] += 1;
            if (v < a.deg.size()) s[v] = std::min(s[v], a.deg[v]);
            if (v < b.deg.size()) s[v] = std::min(s[v], b.deg[v]);
        }
        return s;
    }
    static void broadcast(P& x, P& y) {
        if (x.deg.size() < y.deg.size()) x.deg.insert(x.deg.end(), y.deg.begin() + x.deg.size(), y.deg.end());
        else if (y.deg.size() < x.deg.size()) y.deg.insert(y.deg.end(), x.deg.begin() + y.deg.size(), x.deg.end());
        while (x.shape.size() < y.shape.size()) x.shape.push_back(1);
        while (y.shape.size() < x.shape.size()) y.shape.push_back(1);
    }

    // ---- structured copies -----------------------------------------------------------------------
    // General gather of `src` into a fresh tensor of shape `out_shape`; per-axis shift and valid length.
    // `tier`: -1 = decide here; callers that pass `tab` / `keep` pointers decide first (gather_tier) and pass the
    // pointers of that side.
    static bool gather_tier(const P& src, const Dims& out_shape) { return tier_host(prod(out_shape), src); }
    static P gather(const P& src, const Dims& out_shape, const Dims& out_deg, const Shifts& shift,
                    const Dims& src_len, int op = OP_COPY, const double* s = nullptr, int tab_axis = -1,
                    const double* tab = nullptr, size_t tab_plane = 0, const unsigned char* keep = nullptr, int tier = -1) {
        const bool host = tier < 0 ? gather_tier(src, out_shape) : tier != 0;
        if (!host && !tab && !keep && (op == OP_COPY || op == OP_MUL_S || op == OP_DIV_S || op == OP_NEG || op == OP_LMUL_S) &&
            can_defer(src, prod(out_shape))) {
            // a box of src that lies wholly inside it (no zero padding), optionally mapped elementwise: deferred (no
            // launch).  A box that does not start at element 0 moves the view's origin, which is only meaningful for stages
            // that do not look at positions: a chain holding FIRST / table stages is materialised first.
            bool inside = out_shape.size() <= src.shape.size(), shifted = false;
            for (size_t ax = 0; ax < out_shape.size() && inside; ++ax) {
                if (shift[ax] < 0 || (size_t)shift[ax] + out_shape[ax] > std::min(src_len[ax], src.shape[ax])) inside = false;
                if (shift[ax] != 0) shifted = true;
            }
            if (inside && shifted && src.pend)
                for (int i = 0; i < src.pend->n; ++i)
                    if (src.pend->st[i].kind >= CH_FIRST_ADD) inside = false;  // FIRST_* and MUL_TAB are positional
            // zeros in front (mul_var: shift -1 along one axis, the source cut at src_len): the same view with a pad
            bool front = !inside && out_shape.size() <= src.shape.size();
            if (front) {
                bool any_neg = false;
                for (size_t ax = 0; ax < out_shape.size() && front; ++ax) {
                    if (shift[ax] > 0) front = false;
                    if (shift[ax] < 0) any_neg = true;
                }
                if (!any_neg) front = false;
                // (positional stages of the source chain — FIRST_*, MUL_TAB — are evaluated in the view's own coordinates
                // by k_chain, so they ride along under the pad; a pad on a pad is materialised by deferred())
                if (front && src.pend && src.pend->padded) front = false;
            }
            if (front) {
                P r = deferred(src, out_shape, out_deg, op == OP_COPY ? 0 : 1);
                if (op != OP_COPY) push_stage(r, op == OP_MUL_S ? CH_MUL_S : (op == OP_DIV_S ? CH_DIV_S : (op == OP_NEG ? CH_NEG : CH_LMUL_S)), s);
                Pend& q = *r.pend;
                q.padded = true;
                q.pad = Dims(out_shape.size(), 0);
                q.src_box = Dims(out_shape.size(), 0);
                for (size_t ax = 0; ax < out_shape.size(); ++ax) {
                    q.pad[ax] = (size_t)(-shift[ax]);
                    q.src_box[ax] = std::min(src_len[ax], src.shape[ax]);
                }
                r.c0_known = true;  // element 0 lies in the padding
                r.c0[0] = r.c0[1] = 0.0;
                return r;
            }
            if (inside) {
                P r = deferred(src, out_shape, out_deg, op == OP_COPY ? 0 : 1);
                if (shifted) {
                    const Dims& bs = r.pend->base_shape;
                    size_t stride = 1, off = 0;
                    for (size_t ax = bs.size(); ax-- > 0;) {
                        if (ax < out_shape.size()) off += (size_t)shift[ax] * stride;
                        stride *= bs[ax];
                    }
                    r.pend->base_off += off;
                    r.c0_known = false;  // element 0 is another element now
                }
                if (op != OP_COPY) push_stage(r, op == OP_MUL_S ? CH_MUL_S : (op == OP_DIV_S ? CH_DIV_S : (op == OP_NEG ? CH_NEG : CH_LMUL_S)), s);
                return r;
            }
        }
        P out = make(out_shape, out_deg, host);
        if (out.numel == 0) return out;
        if (W == 2 && !host && !tab && !keep && (op == OP_COPY || op == OP_MUL_S || op == OP_DIV_S || op == OP_NEG || op == OP_LMUL_S) &&
            !((op == OP_MUL_S || op == OP_LMUL_S) && s && !scale_keeps_zero_pattern(s)) && !(op == OP_DIV_S && s && !quotient_keeps_zero_pattern(s))) {
            // (round 6, Support) a box of the source that lies inside it keeps the source's zero pattern, seen from its own origin
            Support sp = support_of_poly<E>(src);
            bool inside = sp.exact() && out_shape.size() <= src.shape.size() && out_shape.size() <= (size_t)Buf::ZAX;
            for (size_t ax = 0; ax < out_shape.size() && inside; ++ax) {
                if (shift[ax] < 0 || (size_t)shift[ax] + out_shape[ax] > std::min(src_len[ax], src.shape[ax])) inside = false;
                else {
                    sp.z[ax] = sp.z[ax] > (size_t)shift[ax] ? (unsigned)(sp.z[ax] - (size_t)shift[ax]) : 0u;
                    if (sp.z[ax] > 0 && sp.z[ax] >= out_shape[ax]) sp.kind = 5;
                }
            }
            for (size_t ax = out_shape.size(); ax < src.shape.size() && inside; ++ax)
                if (src.shape[ax] != 1) inside = false;
            if (inside) {
                if (sp.kind != 5) {
                    sp.kind = 3;
                    sp.normalise();
                }
                sp.store(out.buf.get());
            }
        }
        Dims sst = c_strides(src.shape);
        // collapse axes that are trivial in the output and read index 0 (+shift) of the source
        GatherArgs a;
        std::memset(&a, 0, sizeof(a));
        int nd = 0;
        size_t base = 0;
        a.tab_axis = -1;
        for (size_t ax = 0; ax < out_shape.size(); ++ax) {
            if (out_shape[ax] == 1 && (int)ax != tab_axis) {
                long long si = shift[ax];
                if (si < 0 || (size_t)si >= src_len[ax]) {  // whole output is outside the source box
                    zero_elems(host, tp<E>(out, host), out.numel * W);
                    return seal(out);
                }
                base += (size_t)si * sst[ax];
                continue;
            }
            if (nd >= MAXD) throw Error("tensor rank exceeds GFT MAXD after collapsing");
            a.out.d[nd] = (unsigned)out_shape[ax];
            a.shift[nd] = (int)shift[ax];
            a.src_len[nd] = (unsigned)std::min<size_t>(src_len[ax], 0xffffffffu);
            a.src_stride[nd] = sst[ax];
            if ((int)ax == tab_axis) a.tab_axis = nd;
            nd++;
        }
        // merge adjacent axes that are unmasked and contiguous in the source (elementwise maps become 1-D,
        // slab ops 3-D): less index arithmetic per element, longer unit-stride runs for 16-byte accesses
        for (int i = nd - 1; i >= 1;) {
            int o = i - 1;
            bool ok = a.shift[o] == 0 && a.shift[i] == 0 && a.out.d[o] <= a.src_len[o] && a.out.d[i] <= a.src_len[i] &&
                      a.src_stride[o] == (size_t)a.out.d[i] * a.src_stride[i] && o != a.tab_axis && i != a.tab_axis &&
                      (unsigned long long)a.out.d[o] * a.out.d[i] <= 0xffffffffull;
            if (ok) {
                a.out.d[o] = a.out.d[o] * a.out.d[i];
                a.src_len[o] = a.out.d[o];
                a.src_stride[o] = a.src_stride[i];
                for (int j = i; j + 1 < nd; ++j) {
                    a.out.d[j] = a.out.d[j + 1];
                    a.shift[j] = a.shift[j + 1];
                    a.src_len[j] = a.src_len[j + 1];
                    a.src_stride[j] = a.src_stride[j + 1];
                }
                if (a.tab_axis > i) a.tab_axis--;
                nd--;
            }
            i--;
        }
        a.out.nd = nd;
        a.op = op;
        if (s) {
            a.s.a = s[0];
            a.s.b = W == 2 ? s[1] : 0.0;
        }
        a.tab = tab;
        a.tab_plane = tab_plane;
        a.keep = keep;
        if (host) {
            HK<E>::gather(hp<E>(src) + base, src.numel, hp<E>(out), out.numel, a);
            return seal(out);
        }
        K<E>::gather(R.stream, dp<E>(src) + base, src.numel, dp<E>(out), out.numel, a);
        return out;
    }
    static P lead_block(const P& p, const Dims& lens, const Dims& deg) {  // slice 0..lens per axis
        if (lens == p.shape) return with_meta(p, p.shape, deg);
        Shifts shift(lens.size(), 0);
        return gather(p, lens, deg, shift, p.shape);
    }
    static P slab_range(const P& p, size_t v, size_t lo, size_t hi, const Dims& deg, int op = OP_COPY,
                        int tab_axis = -1, const double* tab = nullptr, size_t tab_plane = 0, int tier = -1) {
        Dims out = p.shape;
        out[v] = hi - lo;
        Shifts shift(out.size(), 0);
        shift[v] = (long long)lo;
        return gather(p, out, deg, shift, p.shape, op, nullptr, tab_axis, tab, tab_plane, nullptr, tier);
    }
    // truncate_degrees on a handle the caller owns: where nothing is cut off (the common case) only the degrees change, in place
    static void truncate_here(P& p, const Dims& degs) {
        bool clip = false;
        for (size_t v = 0; v < p.deg.size(); ++v)
            if (v < p.shape.size() && p.shape[v] > degs[v]) clip = true;
        if (clip) {
            p = truncate_degrees(p, degs);
            return;
        }
        for (size_t v = 0; v < p.deg.size(); ++v)
            if (degs[v] < p.deg[v]) p.deg[v] = degs[v];
        check_invariants(p.shape, p.deg);
    }
    static P truncate_degrees(const P& p, const Dims& degs) {  // mt:195-204
        Dims nd = p.deg, lens = p.shape;
        for (size_t v = 0; v < p.deg.size(); ++v) {
            nd[v] = std::min(nd[v], degs[v]);
            if (v < lens.size() && lens[v] > degs[v]) lens[v] = degs[v];
        }
        return lead_block(p, lens, nd);
    }
    static P map_copy(const P& p, int op, const double* s) {  // fresh tensor = f(p) elementwise
        if (p.numel == 1 && p.cached && (op == OP_LMUL_S || op == OP_MUL_S || op == OP_DIV_S || op == OP_NEG)) {
            // both operands are host-known scalars: one IEEE operation on the host (what the reference does,
            // mt:1033-1047), no launch, no buffer — the result is again a lazy scalar
            int kind = op == OP_LMUL_S ? IMM_LMUL : (op == OP_MUL_S ? IMM_MUL : (op == OP_DIV_S ? IMM_DIV : IMM_NEG));
            Scalar2 b{s ? s[0] : 0.0, (s && W == 2) ? s[1] : 0.0};
            return from_host_value(HK<E>::scalar_imm(kind, E::from(Scalar2{p.cv[0], p.cv[1]}), E::from(b)), p.shape, p.deg);
        }
        Shifts shift(p.shape.size(), 0);
        return gather(p, p.shape, p.deg, shift, p.shape, op, s);
    }

    // ---- constructors (mt:208-259) ------------------------------------------------------------------
    static P zero_with(const Dims& deg) {
        double z[2] = {0, 0};
        return from_host_scalar(z, Dims(deg.size(), 1), deg);
    }
    static P scalar(const double* x) { return from_host_scalar(x, {}, {}); }
    static P var_like(size_t v, const double* x, bool have_x, size_t len_v_shape, bool second_is_one, const Dims& deg) {
        Dims shape(deg.size(), 1);
        shape[v] = len_v_shape;
        check_invariants(shape, deg);
        P r;  // lazy (see gft_poly / dp()): nothing is launched here
        r.width = W;
        r.shape = shape;
        r.deg = deg;
        r.numel = prod(shape);  // 1 or 2
        Scalar2 v0{0.0, 0.0}, v1{0.0, 0.0};
        if (have_x) v0 = Scalar2{x[0], W == 2 ? x[1] : 0.0};
        if (r.numel == 2 && second_is_one) v1 = Scalar2{1.0, 1.0};
        r.cv[0] = v0.a;
        r.cv[1] = W == 2 ? v0.b : 0.0;
        if (r.numel == 2) {  // x + 1*eps_v (or 0*eps_v): its extract_linear verdict is known from the host values
            r.lazy_lin = true;
            r.cv1[0] = v1.a;
            r.cv1[1] = W == 2 ? v1.b : 0.0;
            r.lazy_var = v;
        } else {
            r.cached = true;
        }
        return r;
    }

    // the two-element tensor c = [e0, e1] (planes 2 doubles apart) along axis v as a lazy handle (gft_from_host)
    static P affine_like(size_t v, const double* c, const Dims& shape, const Dims& deg) {
        check_invariants(shape, deg);
        P r;
        r.width = W;
        r.shape = shape;
        r.deg = deg;
        r.numel = 2;
        r.lazy_lin = true;
        r.lazy_var = v;
        r.cv[0] = c[0];
        r.cv1[0] = c[1];
        r.cv[1] = W == 2 ? c[2] : 0.0;
        r.cv1[1] = W == 2 ? c[3] : 0.0;
        return r;
    }
    // lazy (0 + m*eps_v) (+|-) cached scalar d -> lazy (d or -d) + m*eps_v; false if the constant is not an exact zero
    static bool lazy_zero_plus(const P& lazy, const P& scalar, bool subtract, P* out) {
        const double d0 = scalar.cv[0], d1 = scalar.cv[1];
        if (W == 1) {
            if (lazy.cv[0] != 0.0) return false;
            double r;
            if (d0 != 0.0 || d0 != d0) r = subtract ? -d0 : d0;  // 0 +/- d (NaN stays NaN)
            else {
                // signed zeros: (+0)+(+0)=+0, (+0)+(-0)=+0, (-0)+(-0)=-0, (-0)+(+0)=+0; x - y = x + (-y)
                bool ns = std::signbit(lazy.cv[0]), nd = std::signbit(d0) != subtract;
                r = (ns && nd) ? -0.0 : 0.0;
            }
            P res = lazy;
            res.cv[0] = r;
            *out = res;
            return true;
        }
        if (!(lazy.cv[0] == 0.0 && lazy.cv[1] == 0.0)) return false;
        P res = lazy;
        if (subtract) {  // add(a, neg(b)) with a == 0 -> neg(b) = (-hi, -lo)
            res.cv[0] = -d1;
            res.cv[1] = -d0;
        } else {
            res.cv[0] = d0;
            res.cv[1] = d1;
        }
        *out = res;
        return true;
    }

    // A recorded Add / Sub of two chains (addsub's chain path): the operands as they stood after broadcast and truncation.
    struct LazySum {
        P a, b;
        bool subtract = false;
        Dims shape;  // the sum's own shape
    };
    static void launch_sum(const LazySum& ls, double* outp) {
        Dims ckeep = chain_keep(ls.shape, {&ls.a, &ls.b});
        if (!ls.a.pend) (void)dp<E>(ls.a);
        if (!ls.b.pend) (void)dp<E>(ls.b);
        Shape sh;
        sh.nd = (int)ckeep.size();
        for (size_t j = 0; j < ckeep.size(); ++j) sh.d[j] = (unsigned)ls.shape[ckeep[j]];
        K<E>::chain_addsub(R.stream, outp, prod(ls.shape), sh, chain_src_dev(ls.a, ckeep), chain_src_dev(ls.b, ckeep), ls.subtract ? 1 : 0);
        R.stats_ex[2]++;
    }
    // addsub(self, other) where an operand is (a stage-carrying whole view of) a recorded sum: ONE launch evaluates the recorded
    // sum(s) and this one, element for element the operations of the separate launches (K<E>::chain_nest).  false = not this
    // case (nothing launched).
    static bool fuse_lazy_sums(const P& self, const P& other, bool subtract, const Dims& shape, const Dims& rd, P* result) {
        if (!R.lazy_sum) return false;
        auto sum_of = [&](const P& p) -> LazySum* {
            if (!p.buf || p.buf->host || !p.buf->lazy || !p.buf->lazy->sum) return nullptr;
            LazySum* ls = static_cast<LazySum*>(p.buf->lazy->sum.get());
            if (!same_dims_mod_trailing_ones(p.shape, ls->shape)) return nullptr;  // (a sub-box view: launch the sum)
            if (p.pend) {
                const Pend& q = *p.pend;
                if (q.padded || q.base_off != 0 || q.mat || !same_dims_mod_trailing_ones(q.base_shape, ls->shape)) return nullptr;
                for (int i = 0; i < q.n; ++i)
                    if (q.st[i].kind == CH_MUL_TAB) return nullptr;  // (table stages index the view's axes: keep it simple)
            }
            return ls;
        };
        LazySum* la = sum_of(self);
        LazySum* lb = sum_of(other);
        if (!la && !lb) return false;
        if (la && lb && self.buf.get() == other.buf.get()) return false;
        // the kernel's axes: the output's non-unit axes and every table / pad axis of the four leaves
        Dims keep;
        {
            std::vector<const P*> leaves;
            auto add_leaves = [&](const P& p, LazySum* l) {
                if (l) {
                    leaves.push_back(&l->a);
                    leaves.push_back(&l->b);
                } else
                    leaves.push_back(&p);
            };
            add_leaves(self, la);
            add_leaves(other, lb);
            for (size_t ax = 0; ax < shape.size(); ++ax) {
                bool k = shape[ax] != 1;
                for (const P* p : leaves)
                    if (p->pend) {
                        for (int i = 0; i < p->pend->n; ++i)
                            if (p->pend->st[i].kind == CH_MUL_TAB && (size_t)p->pend->st[i].axis == ax) k = true;
                        if (p->pend->padded && ax < p->pend->pad.size() && p->pend->pad[ax] > 0) k = true;
                    }
                if (k) keep.push_back(ax);
            }
            for (const P* p : leaves) {  // no leaf may index an axis beyond the output's rank
                if (p->pend)
                    for (int i = 0; i < p->pend->n; ++i)
                        if (p->pend->st[i].kind == CH_MUL_TAB && (size_t)p->pend->st[i].axis >= shape.size()) return false;
            }
        }
        if (keep.size() > (size_t)MAXD || prod(shape) >= 0x7fffffffull) return false;
        // hold the recordings: bringing a leaf into memory may launch other recordings, never these (they are not in any rider list)
        Rc<LazyOp> keep_a = la ? self.buf->lazy : nullptr, keep_b = lb ? other.buf->lazy : nullptr;
        if (R.batch_dag) {  // a node of the launch graph (the leaves' geometry is known now, their memory when the level is issued)
            auto fits_meta = [&](const P& p) {
                const ChainSrc c = chain_src<E>(p, keep, false);
                unsigned long long span = 1;
                for (size_t j = 0; j < keep.size(); ++j) span += (unsigned long long)(c.box[j] ? c.box[j] - 1 : 0) * c.stride[j];
                return span < 0x7fffffffull;
            };
            auto all_fit = [&](const P& p, LazySum* l) { return l ? (fits_meta(l->a) && fits_meta(l->b)) : fits_meta(p); };
            if (!all_fit(self, la) || !all_fit(other, lb)) return false;
            auto rec = rc_allocate<NestRec>(gft_small::Alloc<NestRec>());
            rec->self = self;
            rec->other = other;
            rec->keep_a = keep_a;
            rec->keep_b = keep_b;
            rec->shape = shape;
            rec->keep = keep;
            rec->subtract = subtract;
            P out = make_recorded(shape, rd);
            sum_nz_store(self, other, shape, out.buf.get());
            out.buf->lazy = op_of(rec);
            *result = out;
            return true;
        }
        auto leaf = [&](const P& p) {
            if (!p.pend) (void)dp<E>(p);
            return chain_src_dev(p, keep);
        };
        auto fits = [&](const ChainSrc& c) {
            unsigned long long span = 1;
            for (size_t j = 0; j < keep.size(); ++j) span += (unsigned long long)(c.box[j] ? c.box[j] - 1 : 0) * c.stride[j];
            return span < 0x7fffffffull;
        };
        auto nest = [&](const P& p, LazySum* l, NestSrc& n) -> bool {
            std::memset(&n, 0, sizeof(n));
            if (!l) {
                n.nested = 0;
                n.a = leaf(p);
                return fits(n.a);
            }
            n.nested = 1;
            n.sub_inner = l->subtract ? 1 : 0;
            n.a = leaf(l->a);
            n.b = leaf(l->b);
            for (size_t j = 0; j < keep.size(); ++j) n.box[j] = (unsigned)(keep[j] < l->shape.size() ? l->shape[keep[j]] : 1);
            if (p.pend) {
                n.npost = p.pend->n;
                for (int i = 0; i < p.pend->n; ++i) {
                    n.post[i].kind = p.pend->st[i].kind;
                    n.post[i].s = Scalar2{p.pend->st[i].s[0], p.pend->st[i].s[1]};
                }
            }
            return fits(n.a) && fits(n.b);
        };
        NestSrc na, nb;
        if (!nest(self, la, na) || !nest(other, lb, nb)) return false;  // (leaves brought into memory stay there: no harm)
        // (a leaf's dp() may have launched one of the recordings after all — as a leaf of itself it cannot, but be safe)
        if ((la && !self.buf->lazy) || (lb && !other.buf->lazy)) return false;
        P out = make(shape, rd);
        sum_nz_store(self, other, shape, out.buf.get());
        Shape sh;
        sh.nd = (int)keep.size();
        for (size_t j = 0; j < keep.size(); ++j) sh.d[j] = (unsigned)shape[keep[j]];
        K<E>::chain_nest(R.stream, dp<E>(out), out.numel, sh, na, nb, subtract ? 1 : 0);
        R.stats_ex[2]++;
        R.stats_sum++;
        *result = out;
        return true;
    }
    // (intervals) a sum of two tensors of the result's own shape: [0,0] only where both are
    // (round 6: with Supports — the union of two "leading zero slabs" patterns over the whole box is the smaller of the two when
    // one contains the other; a front-padded operand (kind 4: zero AT LEAST there) can only be the contained one)
    static Support sum_support(const P& a, const P& b, const Dims& shape) {
        Support r;
        if (W != 2) return r;
        const Support x = support_of_poly<E>(a), y = support_of_poly<E>(b);
        // each operand's non-zero coefficients as a box lo <= k < hi of the sum's index space (interval sums do not cancel: the
        // sum is zero exactly where both operands are); the union of two boxes is a box when they agree on all axes but one and
        // touch or overlap on that one, or when one contains the other
        struct Box {
            bool known = false, empty = false;
            unsigned lo[Buf::ZAX], hi[Buf::ZAX];
        };
        auto box_of = [&](const Support& sp, const P& p) {
            Box bx;
            if (sp.kind == 5) {
                bx.known = bx.empty = true;
                return bx;
            }
            if (!(sp.kind == 2 || sp.kind == 3 || sp.kind == 4)) return bx;
            for (size_t u = Buf::ZAX; u < p.shape.size(); ++u)
                if (p.shape[u] != 1) return bx;
            bx.known = true;
            for (int u = 0; u < Buf::ZAX; ++u) {
                const unsigned ext = (size_t)u < p.shape.size() ? (unsigned)std::min<size_t>(p.shape[u], 0xfffffffeu) : 1u;
                bx.lo[u] = sp.z[u];
                bx.hi[u] = sp.kind == 4 ? std::min(sp.h[u], ext) : ext;
                if (bx.lo[u] >= bx.hi[u]) bx.empty = true;
            }
            return bx;
        };
        const Box A = box_of(x, a), B = box_of(y, b);
        auto full = [&](const Box& bx) {  // no coefficient of the sum's box is zero in this operand: none is in the sum
            if (!bx.known || bx.empty) return false;
            for (int u = 0; u < Buf::ZAX; ++u) {
                const unsigned ext = (size_t)u < shape.size() ? (unsigned)std::min<size_t>(shape[u], 0xfffffffeu) : 1u;
                if (bx.lo[u] != 0 || bx.hi[u] != ext) return false;
            }
            for (size_t u = Buf::ZAX; u < shape.size(); ++u)
                if (shape[u] != 1) return false;
            return true;
        };
        if (full(A) || full(B)) return Support{2};
        if (!A.known || !B.known) {
            if (g_scan_trace.on) {
                char key[160];
                snprintf(key, sizeof key, "sum_support -> unknown: x.kind=%d (nz %d pend %d) y.kind=%d (nz %d pend %d)", x.kind, a.buf ? (int)a.buf->nz : -1, (int)(a.pend != nullptr), y.kind,
                         b.buf ? (int)b.buf->nz : -1, (int)(b.pend != nullptr));
                g_scan_trace.counts[key]++;
            }
            return r;
        }
        Box U;
        U.known = true;
        auto contains = [](const Box& p, const Box& q) {
            for (int u = 0; u < Buf::ZAX; ++u)
                if (q.lo[u] < p.lo[u] || q.hi[u] > p.hi[u]) return false;
            return true;
        };
        if (A.empty && B.empty) return Support{5};
        if (A.empty || (!B.empty && contains(B, A))) U = B;
        else if (B.empty || contains(A, B)) U = A;
        else {
            int diff = -1;
            for (int u = 0; u < Buf::ZAX; ++u)
                if (A.lo[u] != B.lo[u] || A.hi[u] != B.hi[u]) {
                    if (diff >= 0) return r;  // (they differ on two axes: an L-shaped union)
                    diff = u;
                }
            if (std::max(A.lo[diff], B.lo[diff]) > std::min(A.hi[diff], B.hi[diff])) return r;  // (a gap between them)
            U = A;
            U.lo[diff] = std::min(A.lo[diff], B.lo[diff]);
            U.hi[diff] = std::max(A.hi[diff], B.hi[diff]);
        }
        // storable when the box reaches the end of the sum's own box on every axis: "leading zero slabs"
        for (int u = 0; u < Buf::ZAX; ++u) {
            const unsigned ext = (size_t)u < shape.size() ? (unsigned)std::min<size_t>(shape[u], 0xfffffffeu) : 1u;
            if (U.hi[u] != ext) return r;
            r.z[u] = U.lo[u];
        }
        for (size_t u = Buf::ZAX; u < shape.size(); ++u)
            if (shape[u] != 1) return Support{0};
        r.kind = 3;
        r.normalise();
        return r;
    }
    static void sum_nz_store(const P& a, const P& b, const Dims& shape, Buf* out) { sum_support(a, b, shape).store(out); }
    // ---- Add / Sub / Neg (mt:854-937) -----------------------------------------------------------------
    static P addsub(P self, P other, bool subtract) {
        Dims rd = min_degrees(self, other);
        broadcast(self, other);
        truncate_here(self, rd);
        truncate_here(other, rd);
        // a host-cached scalar operand travels as a kernel argument (no device read, no materialisation)
        auto sptr = [](const P& s) -> const double* { return (s.cached && !s.buf) ? nullptr : dp<E>(s); };
        if (other.numel == 1) {
            // (c + m*eps_v) - c for a still-lazy variable and the host-cached scalar c it was built from (the
            // reference's Subst evaluation: subst - constant_term(subst)): x - x = +0 exactly for finite x, so the
            // result stays lazy as 0 + m*eps_v.  F64 only (an interval difference widens).
            if (W == 1 && subtract && !self.buf && self.lazy_lin && other.cached && !other.buf && std::isfinite(self.cv[0]) &&
                std::memcmp(&self.cv[0], &other.cv[0], sizeof(double)) == 0 && self.deg == rd) {
                P r = self;
                r.cv[0] = 0.0;
                return r;
            }
            // (0 + m*eps_v) +/- d for a still-lazy variable with an exactly zero constant and a host-cached scalar d:
            // 0 + d = d, 0 - d = -d (IEEE identities; interval.rs:126-155 returns the other operand for an exact
            // zero), so `Var(x) + Const(d)` substitutions never touch the device before they are consumed.
            if (!self.buf && self.lazy_lin && other.cached && !other.buf && self.deg == rd && lazy_zero_plus(self, other, subtract, &self))
                return self;
            if (self.numel == 1 && self.cached && other.cached)  // two host-known scalars (mt:862-869): host arithmetic
                return from_host_value(HK<E>::scalar_imm(subtract ? IMM_SUB : IMM_ADD, E::from(Scalar2{self.cv[0], self.cv[1]}),
                                                         E::from(Scalar2{other.cv[0], other.cv[1]})), self.shape, rd);
            if (other.cached && tier_host(self.numel, self)) {
                P out = make(self.shape, rd, true);
                HK<E>::copy_first(hp<E>(self), self.numel, hp<E>(out), out.numel, self.numel, subtract ? FIRST_SUB : FIRST_ADD,
                                  Scalar2{other.cv[0], other.cv[1]});
                return seal(out);
            }
            if (other.cached && can_defer(self, self.numel)) {  // element 0 (+|-) a host-known scalar: one more stage
                P r = deferred(self, self.shape, rd, 1);
                push_stage(r, subtract ? CH_FIRST_SUB : CH_FIRST_ADD, other.cv);
                return r;
            }
            P out = make(self.shape, rd);
            K<E>::copy_first(R.stream, dp<E>(self), self.numel, dp<E>(out), out.numel, self.numel,
                             subtract ? FIRST_SUB : FIRST_ADD, sptr(other), other.numel, Scalar2{other.cv[0], other.cv[1]});
            if (W == 1 && subtract && self.c0_known && other.cached && std::isfinite(self.c0[0]) &&
                std::memcmp(&self.c0[0], &other.cv[0], sizeof(double)) == 0) {
                out.c0_known = true;  // x - x = +0 exactly: the device computes it, the host merely knows the outcome
                out.c0[0] = out.c0[1] = 0.0;
            }
            return out;
        }
        if (self.numel == 1) {
            if (!subtract && !other.buf && other.lazy_lin && self.cached && !self.buf && other.deg == rd &&
                lazy_zero_plus(other, self, false, &other))
                return other;
            if (self.cached && tier_host(other.numel, other)) {
                P out = make(other.shape, rd, true);
                HK<E>::copy_first(hp<E>(other), other.numel, hp<E>(out), out.numel, other.numel,
                                  subtract ? FIRST_SUB_NEG_ALL : FIRST_ADD, Scalar2{self.cv[0], self.cv[1]});
                return seal(out);
            }
            if (self.cached && can_defer(other, other.numel)) {
                P r = deferred(other, other.shape, rd, 1);
                push_stage(r, subtract ? CH_FIRST_SUB_NEG_ALL : CH_FIRST_ADD, self.cv);
                return r;
            }
            P out = make(other.shape, rd);
            K<E>::copy_first(R.stream, dp<E>(other), other.numel, dp<E>(out), out.numel, other.numel,
                             subtract ? FIRST_SUB_NEG_ALL : FIRST_ADD, sptr(self), self.numel, Scalar2{self.cv[0], self.cv[1]});
            return out;
        }
        Dims shape = max_shape(self, other);
        const bool host = tier_host(prod(shape), self, other);
        auto recorded = [](const P& p) { return p.buf && !p.buf->host && p.buf->lazy; };
        if (!host && (self.pend || other.pend || recorded(self) || recorded(other))) {
            // deferred operands: their chains are evaluated inside the add itself (one launch for the whole run of
            // operations that led here)
            Dims ckeep = chain_keep(shape, {&self, &other});
            if (ckeep.size() <= (size_t)MAXD) {
                P fused;
                if (fuse_lazy_observe(self, other, subtract, shape, rd, &fused)) return fused;
                if (fuse_lazy_sums(self, other, subtract, shape, rd, &fused)) return fused;
                const bool shifted = (self.pend && self.pend->padded) || (other.pend && other.pend->padded);
                const bool record = R.lazy_sum && ((prod(shape) >= 64 && shifted) || (R.batch_dag && prod(shape) >= 4));
                P out = record ? make_recorded(shape, rd) : make(shape, rd);
                sum_nz_store(self, other, shape, out.buf.get());
                if (record) {
                    // The Add inside mul_linear (c * t + m * shift(t): one operand carries a front pad) is RECORDED, not launched:
                    // if an Add consumes it (the merge of an `if` whose arms both end in `State ~ Bernoulli(p)`), both run as one
                    // launch (fuse_lazy_sums); anybody else launches it through use_buf().  Other two-chain Adds are launched
                    // where they stand: their consumers are observation chains, and a later launch is only less overlap
                    // (mixture f64 0.129 -> 0.145 s with every Add recorded)
                    auto ls = rc_allocate<LazySum>(gft_small::Alloc<LazySum>());
                    ls->a = self;
                    ls->b = other;
                    ls->subtract = subtract;
                    ls->shape = shape;
                    auto op = rc_allocate<LazyOp>(gft_small::Alloc<LazyOp>());
                    op->sum = ls;
                    op->run = [ls](Buf* b) { launch_sum(*ls, b->p); };
                    auto rec = rc_allocate<SumRec>(gft_small::Alloc<SumRec>());
                    rec->ls = ls;
                    op->rec = rec;
                    out.buf->lazy = op;
                    return out;
                }
                if (!self.pend) (void)dp<E>(self);   // plain operands: lazy handles / host-tier tensors get their device buffer
                if (!other.pend) (void)dp<E>(other);
                Shape sh;
                sh.nd = (int)ckeep.size();
                for (size_t j = 0; j < ckeep.size(); ++j) sh.d[j] = (unsigned)shape[ckeep[j]];
                K<E>::chain_addsub(R.stream, dp<E>(out), out.numel, sh, chain_src_dev(self, ckeep), chain_src_dev(other, ckeep), subtract ? 1 : 0);
                R.stats_ex[2]++;
                return out;
            }
        }
        P out = make(shape, rd, host);
        Dims keep = collapse_mask({&shape}, false);
        HV vo = view(out, host), va = view(self, host), vb = view(other, host);
        if (host) {
            HK<E>::addsub_padded(dview(vo, &keep), dview(va, &keep), dview(vb, &keep), subtract ? 1 : 0);
            return seal(out);
        }
        K<E>::addsub_padded(R.stream, dview(vo, &keep), dview(va, &keep), dview(vb, &keep), subtract ? 1 : 0);
        return out;
    }
    static P neg(const P& a) { return map_copy(a, OP_NEG, nullptr); }

    // a + b * from(c) — the accumulation step of the reference's negative-binomial observation (gf.rs:743-746:
    // `sum += term * TaylorPoly::from(lah)`) — in one pass, no intermediate tensor: per element (0 + a) + (c * b), the
    // operations of Mul's constant path (mt:1041-1047) and of Add (mt:873-880) in their order.  Everything that is not
    // the general case (scalar operands, c = 0 / 1 / non-finite) takes the two reference calls.
    static P add_scaled(const P& a, const P& b, const double* c) {
        auto unfused = [&]() { return addsub(a, mul(b, scalar(c)), false); };
        if (a.numel == 1 || b.numel == 1 || val_is_zero(c) || val_is_one(c)) return unfused();
        for (int i = 0; i < W; ++i)
            if (!(c[i] - c[i] == 0.0)) return unfused();
        P self = a, other = b;  // other = b * c has b's shape and degrees
        Dims rd = min_degrees(self, other);
        broadcast(self, other);
        self = truncate_degrees(self, rd);
        other = truncate_degrees(other, rd);
        if (self.numel == 1 || other.numel == 1) return unfused();
        Dims shape = max_shape(self, other);
        const bool host = tier_host(prod(shape), self, other);
        P out = make(shape, rd, host);
        Dims keep = collapse_mask({&shape}, false);
        HV vo = view(out, host), va = view(self, host), vb = view(other, host);
        const Scalar2 cs{c[0], W == 2 ? c[1] : 0.0};
        if (host) {
            HK<E>::add_scaled_padded(dview(vo, &keep), dview(va, &keep), dview(vb, &keep), cs);
            return seal(out);
        }
        K<E>::add_scaled_padded(R.stream, dview(vo, &keep), dview(va, &keep), dview(vb, &keep), cs);
        return out;
    }

    // ---- extract_linear (mt:275-294) --------------------------------------------------------------------
    // extract_linear in two halves (round 4): `begin` answers from the host where it can (done = true) and otherwise launches
    // the device scan WITHOUT waiting for it; `end` waits for the mailbox and memoises the verdict on the buffer.  Between
    // the two the caller may queue work that is guarded on the device by the scan's verdict word (Mailbox::dev_word): the
    // speculative Horner loop runs behind the scan instead of behind a host round trip (horner_speculative).
    struct ScanToken {
        bool done = false, result = false;   // answered without a device scan
        double c[2] = {0, 0}, m[2] = {0, 0};
        size_t var = 0;
        Mailbox mb;
        Dims keep;                           // collapsed axes the kernel's mask bits refer to
        Rc<Buf> buf;            // the buffer the verdict belongs to
    };
    static ScanToken extract_linear_begin(const P& p) {
        ScanToken t;
        unsigned mask = 0;
        for (size_t v = 0; v < p.shape.size(); ++v)
            if (p.shape[v] >= 2) mask |= 1u << v;
        if (!mask) {
            t.done = true;
            return t;
        }
        if (!p.buf && p.lazy_lin) {
            t.done = t.result = true;
            t.c[0] = p.cv[0]; t.c[1] = p.cv[1];
            t.m[0] = p.cv1[0]; t.m[1] = p.cv1[1];
            t.var = p.lazy_var;
            return t;
        }
        if (p.pend && !p.pend->mat) {
            // a deferred chain whose first consumer asks this question: materialise it and scan it in ONE launch
            // (k_chain_scan); the verdict is memoised on the new buffer like any other
            Pend& q = *p.pend;
            Dims ckeep = chain_keep(p.shape, {&p});
            if (ckeep.size() <= (size_t)MAXD && ckeep.size() <= 32) {
                Rc<Buf> outb = alloc_doubles(p.numel * E::W);
                Shape sh;
                sh.nd = (int)ckeep.size();
                unsigned cm = 0;
                for (size_t j = 0; j < ckeep.size(); ++j) {
                    sh.d[j] = (unsigned)p.shape[ckeep[j]];
                    if (p.shape[ckeep[j]] >= 2) cm |= 1u << j;
                }
                t.mb = next_mail();
                g_scan_mail_open = 1;
                K<E>::chain_copy_scan(R.stream, outb->p, p.numel, sh, chain_src<E>(p, ckeep), cm, R.d_flag + 8, t.mb);
                trace_settle();
                R.stats_ex[1]++;
                R.stats[0]++;
                g_scan_trace.hit(p.numel, ckeep.size());
                q.mat = outb;
                q.mat_shape = p.shape;
                p.buf = q.mat;
                p.pend = nullptr;
                t.keep = ckeep;
                t.buf = p.buf;
                return t;
            }
        }
        settle<E>(p);  // the verdict is memoised per buffer: a deferred chain is materialised first
        if (p.buf && p.buf->lin_state) {
            t.done = true;
            t.result = p.buf->lin_state == 2;
            if (t.result) {
                t.c[0] = p.buf->lin_c[0]; t.c[1] = p.buf->lin_c[1];
                t.m[0] = p.buf->lin_m[0]; t.m[1] = p.buf->lin_m[1];
                t.var = p.buf->lin_var;
            }
            return t;
        }
        // kernel works on the collapsed view; map collapsed axis bits back to real axes
        Dims keep = collapse_mask({&p.shape}, false);
        unsigned cmask = 0;
        for (size_t i = 0; i < keep.size(); ++i)
            if (p.shape[keep[i]] >= 2) cmask |= 1u << i;
        t.keep = keep;
        t.buf = p.buf;
        if (p.buf->host) {
            double res[5];
            HV v = view(p, true);
            res[0] = (double)HK<E>::linear_scan(dview(v, &keep), cmask, res + 1, res + 3);  // {mask, c.lo, c.hi, m.lo, m.hi}
            t.done = true;
            finish_scan(t, res);
            return t;
        }
        HV v = view(p);
        DView dv = dview(v, &keep);
        t.mb = next_mail();
        g_scan_mail_open = 1;
        K<E>::linear_scan(R.stream, dv, cmask, R.d_flag + 8, t.mb);  // one launch (state words 8, 9), result by mailbox
        R.stats[0]++;
        g_scan_trace.hit(p.numel, keep.size());
        return t;
    }
    static void finish_scan(ScanToken& t, const double res[5]) {
        const unsigned got = (unsigned)res[0];
        if (!got) {
            t.buf->lin_state = 1;
            t.result = false;
            return;
        }
        size_t ci = 0;
        while (!((got >> ci) & 1u)) ci++;
        t.c[0] = res[1];
        t.c[1] = res[2];
        t.m[0] = res[3];
        t.m[1] = res[4];
        t.var = t.keep[ci];
        t.buf->lin_state = 2;
        t.buf->lin_c[0] = t.c[0]; t.buf->lin_c[1] = t.c[1];
        t.buf->lin_m[0] = t.m[0]; t.buf->lin_m[1] = t.m[1];
        t.buf->lin_var = t.var;
        t.result = true;
    }
    static bool extract_linear_end(ScanToken& t, double c[2], double m[2], size_t* var) {
        if (!t.done) {
            double res[5];
            g_scan_mail_open = 0;
            wait_mail(t.mb, res, 5);
            finish_scan(t, res);
            t.done = true;
        }
        if (t.result) {
            c[0] = t.c[0]; c[1] = t.c[1];
            m[0] = t.m[0]; m[1] = t.m[1];
            *var = t.var;
        }
        return t.result;
    }
    static bool extract_linear(const P& p, double c[2], double m[2], size_t* var) {
        ScanToken t = extract_linear_begin(p);
        return extract_linear_end(t, c, m, var);
    }

    // Inner-axis split for the tiled kernel (gft_conv_tiled.hip, k_pad_rows / k_fold_rows): rank 2/3 whose last axis
    // exceeds the kernel's 128.  Fills the rank-4 problem (pieces, rows.., piece length) into `t` — the piece axis
    // LEADS, which makes it the kernel's wave-uniform axis — and the piece length.
    static bool plan_inner_split(const ConvArgs& a, ConvArgs& t, unsigned* B_out) {
        const int nd = a.nd;
        if (nd != 2 && nd != 3) return false;
        if (a.j0_min || a.j0_excl || a.j0_desc) return false;
        const unsigned zI = a.zs[nd - 1];
        if (zI <= 128) return false;
        // piece length: multiple of 8, <= 64 (2B - 1 <= 127).  P pieces cost P (P + 1) / 2 untruncated B x B piece
        // products for zI^2 / 2 useful ones, and the kernel's efficiency grows with the number of 8-wide output blocks.
        unsigned best = 0;
        double best_score = -1.0;
        for (unsigned B = 64; B >= 32; B -= 8) {
            const double P = (double)((zI + B - 1) / B);
            const double score = (double)zI * zI / (P * (P + 1) * B * B) * (0.45 + 0.55 * B / 64.0);
            if (score > best_score) {
                best_score = score;
                best = B;
            }
        }
        const unsigned B = best;
        t = a;
        t.nd = 4;
        t.xs[0] = (a.xs[nd - 1] + B - 1) / B;
        t.ys[0] = (a.ys[nd - 1] + B - 1) / B;
        t.zs[0] = std::min((zI + B - 1) / B, t.xs[0] + t.ys[0] - 1);  // pieces that receive piece products (the fold knows)
        if (nd == 2) {
            t.xs[1] = t.ys[1] = t.zs[1] = 1;
            t.xs[2] = a.xs[0]; t.ys[2] = a.ys[0]; t.zs[2] = a.zs[0];
            t.slab_axis = 2;
        } else {
            t.xs[1] = a.xs[0]; t.ys[1] = a.ys[0]; t.zs[1] = a.zs[0];
            t.xs[2] = a.xs[1]; t.ys[2] = a.ys[1]; t.zs[2] = a.zs[1];
            t.slab_axis = 1;
        }
        t.xs[3] = B;
        t.ys[3] = B;
        t.zs[3] = 2 * B - 1;
        t.accumulate = 0;  // the fold applies it
        *B_out = B;
        return true;
    }

