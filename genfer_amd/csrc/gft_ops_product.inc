// Part of struct Ops<E> (included inside its body by gft_api.hip): the product (mt:971-1072): dispatcher, slab-range products on the tiled / staged / shallow / line kernels, mul_linear.
// Split out of gft_api.hip in round 6 by concern; no behavioural change (the compiler sees the same token stream).

    // ---- the product (mt:971-1072) --------------------------------------------------------------------------
    // conv: z[slab range] (+)= x (*) y in the reference's summation structure.  `slab_mode` marks a
    // recurrence step (axis 0 is always an "outer" axis, see gft_kernels.hip).
    static void conv(const HV& x, const HV& y, const HV& z, size_t slab_lo, size_t slab_hi, bool accumulate,
                     bool slab_mode, int j0_min, int j0_excl, int j0_desc) {
        Dims keep = collapse_mask({&z.shape}, slab_mode);
        Dims xs = pick(x.shape, keep), ys = pick(y.shape, keep), zs = pick(z.shape, keep);
        if (zs.size() > (size_t)MAXD) throw Error("tensor rank exceeds GFT MAXD after collapsing");
        ConvArgs a;
        std::memset(&a, 0, sizeof(a));
        a.nd = (int)zs.size();
        Dims xst = c_strides(xs), yst = c_strides(ys), zst = c_strides(zs);
        for (int i = 0; i < a.nd; ++i) {
            a.xs[i] = (unsigned)xs[i];
            a.ys[i] = (unsigned)ys[i];
            a.zs[i] = (unsigned)zs[i];
            a.xstr[i] = xst[i];
            a.ystr[i] = yst[i];
            a.zstr[i] = zst[i];
        }
        if (!z.shape.empty() && slab_hi <= slab_lo) return;  // empty slab range
        const bool axis0_kept = !keep.empty() && keep[0] == 0;
        if (a.nd == 0) {
            a.slab_lo = 0;
            a.slab_hi = 1;
        } else if (!axis0_kept) {  // the (unit) leading axis was collapsed away: its only slab is everything
            a.slab_lo = 0;
            a.slab_hi = a.zs[0];
        } else {
            a.slab_lo = (unsigned)slab_lo;
            a.slab_hi = (unsigned)slab_hi;
        }
        a.accumulate = accumulate ? 1 : 0;
        a.j0_min = j0_min;
        a.j0_excl = j0_excl;
        a.j0_desc = j0_desc;
        a.variant = R.conv_variant;
        a.operands_slack = x.slack ? 1 : 0;
        // number of non-unit axes that take part in the reference's "1-d like" inner product
        int first_inner_axis = slab_mode ? 1 : 0;
        int nonunit = 0;
        for (int i = first_inner_axis; i < a.nd; ++i)
            if (a.zs[i] != 1) nonunit++;
        a.inner_from_zero = nonunit >= 1 ? 1 : 0;

        if (z.host) {  // host tier: the reference's loop nest, operands and result in host memory
            if (!x.host || !y.host) throw Error("internal: host-tier product with a device operand");
            HK<E>::conv_naive(x.p, x.plane, y.p, y.plane, z.p, z.plane, a);
            return;
        }
        if (x.host || y.host) throw Error("internal: device product with a host operand");

        // Shallow product (a stencil): few terms per output, HBM-bound streaming work — the reference-order per-output
        // kernel (bit-exact) beats the compute-bound tiled kernel and the barrier-per-step staged one by an order of
        // magnitude there (three_populations' Horner steps: 80 -> 8 us).
        if (R.conv_mode == 0 && R.shallow_max_terms && !slab_mode && !accumulate && a.nd >= 1 && a.slab_lo == 0 && a.slab_hi == a.zs[0]) {
            size_t terms = 1;
            for (int i = 0; i < a.nd; ++i) terms *= std::min(a.xs[i], a.ys[i]);
            if (terms <= R.shallow_max_terms) {
                // (one operand a LINE of 16+ coefficients along an outer axis: the tile form, gft_kernels.hip k_conv_line)
                if (K<E>::conv_line(R.stream, x.p, x.plane, y.p, y.plane, z.p, z.plane, a)) {
                    R.stats[5]++;
                    R.stats_shallow[0]++;
                    return;
                }
                ConvEpi e;
                std::memset(&e, 0, sizeof(e));
                for (int i = 0; i < a.nd; ++i) e.os[i] = a.zs[i];
                if (K<E>::conv_shallow(R.stream, x.p, x.plane, y.p, y.plane, z.p, z.plane, a, e)) {
                    R.stats[5]++;
                    R.stats_shallow[0]++;
                    return;
                }
            }
        }
        // Small plain f64 products: the row-pair form of the reference-order product (gft_conv_staged.hip) is bit-exact AND
        // faster than the tiled kernel there (two launches, no planning: 12^3 38 -> 14 us, 16^3 27 -> 20, 64^2 27 -> 18,
        // 100^2 42 -> 27 us; crossover at ~20^3 resp. ~200^2, profiles/r04/f64_pairs_vs_tiled.txt)
        if (W == 1 && R.conv_mode == 0 && R.pairs_first && !slab_mode && !accumulate && a.slab_lo == 0 && a.slab_hi == a.zs[0] && a.nd >= 2) {
            if (conv_pairs<E>(R.stream, x.p, x.plane, y.p, y.plane, z.p, z.plane, a, a.nd == 2 ? R.pairs_first_max_rank2 : (a.nd == 3 ? R.pairs_first_max : 0.1 * R.pairs_first_max))) {  // (rank 4: 8^4 27 vs 22 us already)
                R.stats[4]++;
                return;
            }
        }
        bool want_tiled = (W == 1) && (R.conv_mode == 0 || R.conv_mode == 2);
        // A recurrence step (one output slab k with j0 >= j0_min and/or j0 < k) is a plain slab product of shifted
        // operand views:  sum_{j0 >= m, j0 <= k - e} x[j0] y[k - j0]  =  slab k - m - e of  x[m:] (*) y[e:]  (e = 1
        // for "exclusive").  Only the slabs that can contribute are part of the views, so uninitialised later slabs of
        // the result (which is also an operand in div/exp/log) are never read.  Not bit-exact (tiled order), so only
        // above the tiled crossover; j0_desc is an ordering, irrelevant here.
        const double *tx = x.p, *ty = y.p;
        double* tz = z.p;
        ConvArgs ash = a;  // the problem handed to the tiled kernel
        bool shifted_empty = false;
        if (want_tiled && (a.j0_min || a.j0_excl || a.j0_desc)) {
            const unsigned m = (unsigned)a.j0_min, e = a.j0_excl ? 1u : 0u;
            // div / log steps (exclusive j0) stay on the reference-order kernel: those recurrences subtract and divide,
            // and a different summation order showed up as 3e-10 relative on near-cancelling coefficients at 64^3 —
            // outside the 1e-10 contract — while their time is dominated by the lower-dimensional divisions anyway.
            // exp steps (all-additive) agree to 1e-14 and run 15x faster at 64^3.
            if (a.nd < 2 || a.slab_hi != a.slab_lo + 1 || a.accumulate || a.j0_excl || R.conv_mode == 2) {
                want_tiled = false;
            } else if (a.slab_lo < m + e || a.xs[0] <= m || a.ys[0] <= e) {
                shifted_empty = true;  // no admissible j0: the slab is zero
            } else {
                const unsigned kp = a.slab_lo - m - e;
                ash.j0_min = ash.j0_excl = ash.j0_desc = 0;
                ash.xs[0] = std::min(a.xs[0] - m, kp + 1);
                ash.ys[0] = std::min(a.ys[0] - e, kp + 1);
                ash.zs[0] = kp + 1;
                ash.slab_lo = kp;
                ash.slab_hi = kp + 1;
                tx = x.p + (size_t)m * a.xstr[0];
                ty = y.p + (size_t)e * a.ystr[0];
                tz = z.p + (size_t)(m + e) * a.zstr[0];
                for (int i = 1; i < a.nd; ++i)  // operands never exceed the (virtual) result
                    if (ash.xs[i] > ash.zs[i] || ash.ys[i] > ash.zs[i]) want_tiled = false;
            }
        }
        if (want_tiled && shifted_empty) {
            HV cur = z.index0(a.slab_lo);
            HIP_OK(hipMemsetAsync(cur.p, 0, sizeof(double) * cur.numel(), R.stream));
            return;
        }
        if (want_tiled && ash.nd > 4 && !ash.accumulate && ash.zs[ash.nd - 1] <= 128 && conv_tiled_high_rank(x, y, z, a, ash, tx, ty, tz)) return;
        if (want_tiled) {
            // rank 2, or a last axis longer than the tiled kernel's 128: split the last axis into (P, B) pieces
            ConvArgs at = ash;
            unsigned B = 0;
            const bool split = plan_inner_split(ash, at, &B);
            if (split) at.operands_slack = 0;  // its operands are zero-padded pieces: packed and scanned (the non-finite verdict)
            size_t need = 0;
            bool ok = true;
            if (R.conv_mode == 0) {
                // auto: below this the bit-exact reference-order kernels are as fast (fixed costs dominate).  Decided
                // from the shapes alone, BEFORE the tiled planner is asked: a plan query builds tables, takes an arena
                // slice and a cache entry, which small ever-changing shapes (Genfer's supports grow statement by
                // statement) would pay for nothing.
                double macs = 1.0;
                for (int i = 0; i < ash.nd; ++i) {
                    double f = 0.5 * (double)ash.zs[i] * (double)std::min(ash.xs[i], ash.ys[i]);
                    if (i == 0 && ash.slab_hi - ash.slab_lo < ash.zs[0]) f = (double)(ash.slab_hi - ash.slab_lo) * std::min(ash.xs[0], ash.ys[0]);
                    macs *= f;
                }
                const double tmin = R.tiled_min_override >= 0 ? R.tiled_min_override : R.tiled_min_macs;
                // rank 2 runs the kernel with a 1 x 64 lane tile (half-empty below 64 rows), split products pay the pad /
                // fold passes: their crossovers sit higher (tools/xover_host.py: 32^2 staged 34 us / tiled 48, 48^2 60 / 44)
                if (macs < tmin * (split ? 10.0 : (ash.nd == 2 ? 4.0 : 1.0))) ok = false;
            }
            if (ok) ok = conv_tiled_f64(R.stream, tx, ty, tz, at, nullptr, 0, &need, nullptr, 0);
            if (ok) {
                R.ensure_conv_ws(need);
                // Zero padding times inf/NaN would create NaNs the reference does not produce.  The verdict stays
                // on the device: the packing/scan kernels stamp R.d_flag[2] with this product's epoch if an
                // operand is not finite; the tiled kernels then leave z alone and the guarded reference-order
                // launch below computes it (and is a no-op otherwise).  No host round trip.
                unsigned* flag = R.next_nf_epoch();
                bool guarded = true;
                if (!split) {
                    bool peeled = false, forked = false;
                    if (!conv_tiled_f64(R.stream, tx, ty, tz, ash, R.conv_ws, R.conv_ws_bytes, &need, flag, R.nf_epoch, &guarded, &peeled, &forked))
                        throw Error("tiled convolution launch failed");
                    if (peeled) R.stats_peeled++;
                    if (forked) R.stats_side[1]++;
                } else {
                    const ConvArgs& a = ash;  // the (possibly shifted) problem; the guarded fallback below uses the original
                    const double* xsrc = tx;
                    const double* ysrc = ty;
                    double* zdst = tz;
                    const int nd = a.nd;
                    size_t xrows = 1, yrows = 1, zrows = 1, zrows_per0 = 1;
                    for (int i = 0; i + 1 < nd; ++i) {
                        xrows *= a.xs[i];
                        yrows *= a.ys[i];
                        zrows *= a.zs[i];
                        if (i > 0) zrows_per0 *= a.zs[i];
                    }
                    const unsigned Px = at.xs[0], Py = at.ys[0], Pz = at.zs[0], RI = 2 * B - 1;
                    Rc<Buf> xt = alloc_doubles(xrows * Px * B), yt = alloc_doubles(yrows * Py * B);
                    Rc<Buf> zt = alloc_doubles(zrows * Pz * RI);
                    tiled_pad_rows_f64(R.stream, xsrc, xt->p, xrows, a.xs[nd - 1], Px, B);
                    tiled_pad_rows_f64(R.stream, ysrc, yt->p, yrows, a.ys[nd - 1], Py, B);
                    if (!conv_tiled_f64(R.stream, xt->p, yt->p, zt->p, at, R.conv_ws, R.conv_ws_bytes, &need, flag, R.nf_epoch))
                        throw Error("tiled convolution launch failed");
                    // rank 2: the slab range is a row range; rank 3: slabs of z.shape[1] rows
                    size_t per0 = nd == 2 ? 1 : zrows_per0;
                    tiled_fold_rows_f64(R.stream, zt->p, zdst, zrows, a.slab_lo * per0, a.slab_hi * per0, Pz, B, a.zs[nd - 1],
                                        a.accumulate, flag, R.nf_epoch);
                }
                R.stats[3]++;
                if (!guarded) return;  // operands read in place: no zero padding, no verdict, nothing to fall back from
                a.guard = flag;
                a.guard_epoch = R.nf_epoch;
                if (!conv_staged<E>(R.stream, x.p, x.plane, y.p, y.plane, z.p, z.plane, a))
                    K<E>::conv_naive(R.stream, x.p, x.plane, y.p, y.plane, z.p, z.plane, a);
                return;
            }
            if (R.conv_mode == 2) throw Error("conv_mode=2 (tiled) requested but the shape is not supported by the tiled kernel");
        }
        if (R.conv_mode == 0 || R.conv_mode == 3) {
            if (conv_staged<E>(R.stream, x.p, x.plane, y.p, y.plane, z.p, z.plane, a)) {
                R.stats[4]++;
                return;
            }
        }
        R.stats[5]++;
        K<E>::conv_naive(R.stream, x.p, x.plane, y.p, y.plane, z.p, z.plane, a);
    }

    // Rank >= 5 on the tiled kernel (the reference's product is rank-generic, mt:984-1012; the kernel takes the last four
    // axes): the leading axes are walked on the host — for every leading output index u and every admissible j <= u one
    // accumulate-mode rank-4 launch  z[u] += x[j] (*) y[u - j]  on the trailing blocks, which are contiguous in the
    // operands' own layout.  Same multiply-adds as the rank-4 kernel performs, summed per u in ascending j: the tiled
    // contract (1e-10), not the reference's order.  false: not worth it / not supported — the caller takes the
    // reference-order kernels.
    static bool conv_tiled_high_rank(const HV& x, const HV& y, const HV& z, const ConvArgs& a, const ConvArgs& ash, const double* tx,
                                     const double* ty, double* tz) {
        const int extra = ash.nd - 4;
        ConvArgs sub;
        std::memset(&sub, 0, sizeof(sub));
        sub.nd = 4;
        double macs = 1.0, lead_pairs = 1.0;
        for (int i = 0; i < ash.nd; ++i) macs *= 0.5 * (double)ash.zs[i] * (double)std::min(ash.xs[i], ash.ys[i]);
        for (int i = 0; i < 4; ++i) {
            sub.xs[i] = ash.xs[extra + i];
            sub.ys[i] = ash.ys[extra + i];
            sub.zs[i] = ash.zs[extra + i];
            sub.xstr[i] = ash.xstr[extra + i];
            sub.ystr[i] = ash.ystr[extra + i];
            sub.zstr[i] = ash.zstr[extra + i];
        }
        sub.slab_lo = 0;
        sub.slab_hi = sub.zs[0];
        sub.variant = ash.variant;
        for (int i = 0; i < extra; ++i) lead_pairs *= 0.5 * (double)ash.zs[i] * (double)std::min(ash.xs[i], ash.ys[i]) + 0.5;
        // every launch must be worth a launch: the trailing rank-4 product above the tiled crossover
        if (R.conv_mode == 0 && macs / lead_pairs < R.tiled_min_macs) return false;
        size_t need = 0;
        if (!conv_tiled_f64(R.stream, tx, ty, tz, sub, nullptr, 0, &need, nullptr, 0)) return false;
        R.ensure_conv_ws(need);
        unsigned* flag = R.next_nf_epoch();
        // odometer over the leading output index u (axis 0 restricted to the slab range) and, inside, over j
        unsigned u[MAXD] = {0}, j[MAXD] = {0};
        for (int i = 0; i < extra; ++i) u[i] = i == 0 ? ash.slab_lo : 0;
        const unsigned u0_hi = ash.slab_hi;
        if (u0_hi <= ash.slab_lo) return true;
        for (;;) {
            size_t zoff = 0;
            unsigned jlo[MAXD], jhi[MAXD];
            bool any = true;
            for (int i = 0; i < extra; ++i) {
                zoff += (size_t)u[i] * ash.zstr[i];
                jlo[i] = u[i] + 1 > ash.ys[i] ? u[i] + 1 - ash.ys[i] : 0;
                jhi[i] = std::min(u[i], ash.xs[i] - 1);
                if (jlo[i] > jhi[i]) any = false;
                j[i] = jlo[i];
            }
            bool first = true;
            if (!any) {  // no admissible j (compact operands): the block is zero
                zero_elems(false, tz + zoff, (size_t)ash.zstr[extra - 1]);
            } else {
                for (;;) {
                    size_t xoff = 0, yoff = 0;
                    for (int i = 0; i < extra; ++i) {
                        xoff += (size_t)j[i] * ash.xstr[i];
                        yoff += (size_t)(u[i] - j[i]) * ash.ystr[i];
                    }
                    sub.accumulate = first ? 0 : 1;
                    first = false;
                    if (!conv_tiled_f64(R.stream, tx + xoff, ty + yoff, tz + zoff, sub, R.conv_ws, R.conv_ws_bytes, &need, flag, R.nf_epoch))
                        throw Error("tiled convolution launch failed");
                    int ax = extra - 1;
                    for (; ax >= 0; --ax) {
                        if (++j[ax] <= jhi[ax]) break;
                        j[ax] = jlo[ax];
                    }
                    if (ax < 0) break;
                }
            }
            int ax = extra - 1;
            for (; ax >= 0; --ax) {
                const unsigned hi = ax == 0 ? u0_hi : ash.zs[ax];
                if (++u[ax] < hi) break;
                u[ax] = ax == 0 ? ash.slab_lo : 0;
            }
            if (ax < 0) break;
        }
        R.stats[3]++;
        // non-finite operands: the tiled launches left z alone from the launch that noticed on; the guarded reference-order
        // launch recomputes ALL of z then (accumulate is off here, so nothing of the earlier partial sums survives)
        ConvArgs g = a;
        g.guard = flag;
        g.guard_epoch = R.nf_epoch;
        if (!conv_staged<E>(R.stream, x.p, x.plane, y.p, y.plane, z.p, z.plane, g))
            K<E>::conv_naive(R.stream, x.p, x.plane, y.p, y.plane, z.p, z.plane, g);
        return true;
    }

    static P mul_var(const P& self, const double* m, size_t v, const Dims& shape, const Dims& deg) {  // mt:589-608
        if (v >= self.shape.size() || shape.size() != self.shape.size()) throw Error("mul_var: bad axis/shape");
        size_t upper = std::min(shape[v] - 1, self.shape[v]);
        Shifts shift(shape.size(), 0);
        shift[v] = -1;
        Dims src_len = self.shape;
        src_len[v] = upper;
        return gather(self, shape, deg, shift, src_len, OP_MUL_S, m);
    }
    static P mul_linear(const P& self, const double* c, const double* m, size_t v, const Dims& shape, const Dims& deg) {  // mt:611-623
        if (val_is_zero(c)) return mul_var(self, m, v, shape, deg);
        return addsub(mul_var(self, m, v, shape, deg), mul(self, scalar(c)), false);
    }

    // c * eps_v for a still-lazy plain variable (0 + 1*eps_v) and a finite host-known scalar c: the result is
    // (c*0, c*1) = (0 with c's sign, c) by IEEE identities (interval: the exact zero / one short-circuits of
    // interval.rs:164-190), so it can stay lazy — and a later subst_var(.., c*eps_v) knows from the host that the
    // substitution is a pure scaling instead of scanning a 2-element device tensor (one host round trip less).
    static bool scaled_lazy_var(const P& var, const double c[2], P* out) {
        if (var.buf || !var.lazy_lin || var.numel != 2) return false;
        auto is_pz = [](double x) { return x == 0.0 && !std::signbit(x); };
        if (!is_pz(var.cv[0]) || var.cv1[0] != 1.0) return false;
        if (W == 2 && (!is_pz(var.cv[1]) || var.cv1[1] != 1.0)) return false;
        if (!std::isfinite(c[0]) || (W == 2 && !std::isfinite(c[1]))) return false;
        P r = var;
        if (W == 1) {
            r.cv[0] = std::copysign(0.0, c[0]);
            r.cv[1] = 0.0;
        } else {
            r.cv[0] = r.cv[1] = 0.0;
        }
        r.cv1[0] = c[0];
        r.cv1[1] = W == 2 ? c[1] : 0.0;
        *out = r;
        return true;
    }

    static P mul(P self, P other) {  // mt:1014-1072
        Dims deg = min_degrees(self, other);
        if (is_zero(self) || is_zero(other)) return zero_with(deg);
        broadcast(self, other);
        Dims shape = sum_shape(self, other);
        truncate_here(self, deg);
        truncate_here(other, deg);
        if (is_one(self)) return other;
        if (is_one(other)) return self;
        double c[2], m[2];
        if (self.numel == 1) {
            first_value(self, c);
            P lazy;
            if (scaled_lazy_var(other, c, &lazy)) return lazy;
            return map_copy(other, OP_LMUL_S, c);
        }
        if (other.numel == 1) {
            first_value(other, c);
            P lazy;
            if (scaled_lazy_var(self, c, &lazy)) return lazy;
            return map_copy(self, OP_LMUL_S, c);
        }
        size_t v;
        ScanCtx sc_self("mul.self");
        if (extract_linear(self, c, m, &v)) {
            Dims sh = other.shape;
            sh[v] = std::min(deg[v], sh[v] + 1);
            return mul_linear(other, c, m, v, sh, deg);
        }
        ScanCtx sc_other("mul.other");
        if (extract_linear(other, c, m, &v)) {
            Dims sh = self.shape;
            sh[v] = std::min(deg[v], sh[v] + 1);
            return mul_linear(self, c, m, v, sh, deg);
        }
        const bool host = tier_host(prod(shape), self, other) && est_macs(self.shape, other.shape, shape) <= R.host_max_macs;
        P out = make(shape, deg, host);
        if (!host && W == 1 && dist_shard(self, other, out)) return out;  // multi-GPU: leading axis sharded (gft_dist_init)
        conv(view(self, host), view(other, host), view(out, host), 0, shape.empty() ? 1 : shape[0], false, false, 0, 0, 0);
        return seal(out);
    }
    static bool dist_shard(const P& self, const P& other, const P& out);  // defined after the RCCL plumbing
    // multiply-adds of a full product, estimated from the shapes (the dispatch criterion for general products)
    static double est_macs(const Dims& xs, const Dims& ys, const Dims& zs) {
        double macs = 1.0;
        int rank = 0;
        for (size_t i = 0; i < zs.size(); ++i) {
            macs *= 0.5 * (double)zs[i] * (double)std::min(xs[i], ys[i]) + 0.5;
            if (zs[i] > 1) rank++;
        }
        return macs * (rank <= 1 ? 1.0 : (rank == 2 ? 1.4 : 2.8));  // host cost in rank-1 multiply-adds (xover_host.txt)
    }

