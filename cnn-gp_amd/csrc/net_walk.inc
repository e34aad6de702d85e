// net_walk.inc — the pair walk of net_kernel (netfuse.hip), included there once per op chain
// with CGP_WALK_LEAN = false / true: a kernel that carries the lean chain of a compiled
// program (kLeanProg) holds two walks behind one workgroup-uniform branch, so neither walk
// carries the other's registers; every other kernel holds this loop once, as before.
// Uses the kernel's locals: p, lds, tid, beg, end, advance, grab, ctr, pair_tab, red_part,
// prog_recs, hx and its template parameters.
    for (long long u = advance(); u < end; u = advance()) {
        if (tid == 0) grab = atomicAdd(ctr, 1ull);
        Pairs pr;
        pr.tab = pair_tab;
        pr.u0 = u;
        pr.red = red_part;
        if constexpr (NP == 2) {
            // one-pair slices sharing the workgroup's barriers: waves 2q, 2q + 1 run unit
            // u + q (the next j of the same image i), each on its own arena.  The pair is
            // uniform per wave, so each slice runs the one-pair code (scalar variance-map
            // bases)
            // every wave decodes the group's units (scalar); the group is skipped only when
            // none of them is evaluated, so all waves agree at every barrier
            const int q = __builtin_amdgcn_readfirstlane(tid >> 7);
            unsigned iq = 0, jq = 0;
            bool vq = false, wq = false, any = false;
#pragma unroll
            for (int s = 0; s < UN; ++s) {
                unsigned is = 0, js = 0;
                const bool vs = u + s < end && unit_pair(p, u + s, is, js);
                const bool ws = vs && !(p.same && js <= is);
                any |= ws;
                if (s == q) {
                    iq = is;
                    jq = js;
                    vq = vs;
                    wq = ws;
                }
            }
            if (!any) {   // below the diagonal of a same tile (or outside): K[i, i] only
                if (p.final_stage && p.same && (tid & (kNT - 1)) == 0 && vq && jq == iq)
                    p.out[(long long)iq * p.ldo + iq] = p.kdiag[iq];
                continue;
            }
            Pairs ph;
            ph.tab = pair_tab;
            ph.u0 = u + q;
            ph.red = red_part + q * (kNT / 64);
            // a slice without a pair computes on clamped indices and stores nothing
            ph.i = __builtin_amdgcn_readfirstlane(vq ? iq : 0u);
            ph.j = __builtin_amdgcn_readfirstlane(vq ? jq : 0u);
            T* lh = lds + q * p.lds_elems;
            const int ht = tid & (kNT - 1);
            if constexpr (PID < 0) {
                for (int k = 0; k < p.nops; ++k) {
                    const cgp_net_op op = load_op(ops_c(p.ops) + k);
                    net_op<T, EX, DU, 1>(lh, op, p, ph, ht);
                    lds_barrier();
                }
            } else {
                prog_ops<T, DU, 1, PID, 0, CGP_WALK_LEAN>(lh, p, ph, ht, prog_recs, hx);
            }
            if (p.final_stage && ht == 0 && vq) {
                if (wq) {
                    const T v = lh[p.final_slot];
                    p.out[(long long)ph.i * p.ldo + ph.j] = v;
                    if (p.same) p.out[(long long)ph.j * p.ldo + ph.i] = v;
                } else if (ph.j == ph.i) {
                    p.out[(long long)ph.i * p.ldo + ph.i] = p.kdiag[ph.i];
                }
            }
        } else {
            if constexpr (NP == 1) {
                if (!unit_pair(p, u, pr.i, pr.j)) continue;
                pr.i = __builtin_amdgcn_readfirstlane(pr.i);   // uniform: scalar map offsets
                pr.j = __builtin_amdgcn_readfirstlane(pr.j);
                if (p.same && pr.j <= pr.i) {
                    if (p.final_stage && pr.j == pr.i && tid == 0)
                        p.out[(long long)pr.i * p.ldo + pr.i] = p.kdiag[pr.i];
                    continue;
                }
            } else {
                // the group's pair table; pairs outside the tile are computed on clamped
                // indices and never stored
                if (tid < NP) {
                    unsigned iq = 0, jq = 0;
                    unit_pair(p, u + tid, iq, jq);
                    pair_tab[tid] = iq < p.n1 ? iq : p.n1 - 1;
                    pair_tab[kMaxNP + tid] = jq < p.n2 ? jq : p.n2 - 1;
                }
                pr.i = pr.j = 0;
                lds_barrier();
            }
            if constexpr (PID < 0) {
                for (int k = 0; k < p.nops; ++k) {
                    const cgp_net_op op = load_op(ops_c(p.ops) + k);
                    net_op<T, EX, DU, NP>(lds, op, p, pr, tid);
                    lds_barrier();
                }
            } else {
                prog_ops<T, DU, NP, PID, 0, CGP_WALK_LEAN>(lds, p, pr, tid, prog_recs, hx);
            }
            if (p.final_stage) {
                if constexpr (NP == 1) {
                    if (tid == 0) {
                        const T v = lds[p.final_slot];
                        p.out[(long long)pr.i * p.ldo + pr.j] = v;
                        if (p.same) p.out[(long long)pr.j * p.ldo + pr.i] = v;
                    }
                } else if (tid < NP) {
                    unsigned iq, jq;
                    if (u + tid < end && unit_pair(p, u + tid, iq, jq)) {
                        if (!p.same || jq > iq) {
                            const T v = lds[tid * p.lds_elems + p.final_slot];
                            p.out[(long long)iq * p.ldo + jq] = v;
                            if (p.same) p.out[(long long)jq * p.ldo + iq] = v;
                        } else if (jq == iq) {
                            p.out[(long long)iq * p.ldo + iq] = p.kdiag[iq];
                        }
                    }
                }
            }
        }
        lds_barrier();
    }
