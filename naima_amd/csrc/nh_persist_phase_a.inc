// nh_persist_phase_a.inc -- phase A of a turn of the resident loop (k_half_step_run, nh_persist.hip):
// wave 0 takes the walker's own and its partner's record from the ring, makes the proposal (emcee
// StretchMove.get_proposal; reference call sites core.py:128, 450-457) and evaluates the parameter
// packs.  Included TWICE: as the turn's own phase A -- inline, every instance: the code it was --
// and as the body of the DEEP instance's lambda that makes the NEXT walker's phase A ahead of time.
// Names it reads: the slice's r, idx, tl, half; j; the small block's qs, row, lg, accs, hi, hx, olds;
// it writes pval, pcol, slice_bad.  HSR_A_AHEAD: "look at the records once, do not wait";
// HSR_A_NOT_YET: what to do then.
      const int g = H.lo + j;
      const int me = idx[g], pa = idx[ns + g];
      const double mz = r[g], mlnu = r[ns + g];
      if (lane == 0) {
        hi[HI_CNT] = 0;
        hi[HI_LIVE] = 0;
        hi[HI_READY] = 0;
        hi[HI_NZ] = 0;
        hi[HI_TICK] = 0;  // (here: the abort flag of this slice)
        if (DEEP) hx[HX_SPECRD] = 0;
      }
      // lanes 0 .. GRn-1: my own record in row tl (the state after the previous step);
      // lanes 32 .. 32+GRn-1: the partner's -- row tl for the first half of a step, row
      // tl + 1 for the second (the partner has moved in the first half of THIS step)
      // this lane's parameter-pack column (walker-independent: read BEFORE the wait for the
      // records, so that what follows their arrival is shuffles and arithmetic only -- the byte
      // of pkd was a vector load from the kernel-argument segment behind the records, the
      // descriptor three dependent LDS trips)
      double pk_a = 0.0, pk_b = 0.0, pk_c = 0.0, pk_lna = 0.0;
      int pk_tf = 0, pk_nc = 0, pkd = -1;
      // (what stands in for ln e when this lane's column is an energy without a logarithm: 0 for a
      // slot the kind leaves unused, NaN for one it uses -- pd_ln_default; walker-independent too)
      const double pk_ln0 = pd_ln_default_flags(H.F.broken, (lane % NH_MAX_LAZY) >> 1);
      if (lane < npk8) {
        const double* o = sm + R.o_pk + lane * HS_RUN_PKW;
        pk_a = o[0]; pk_b = o[1]; pk_c = o[2];
        pk_tf = reinterpret_cast<const int*>(o + 3)[0];
        pk_nc = reinterpret_cast<const int*>(o + 3)[1];
        pk_lna = o[6];
        pkd = reinterpret_cast<const int*>(o + 7)[0];
      }
      const bool mine = lane < GRn, theirs = lane >= 32 && lane - 32 < GRn;
      const int prow = tl + half;
      const unsigned long long* src =
          R.ring + ((long long)(lane < 32 ? tl : prow) * N + (lane < 32 ? me : pa)) * R.gr +
          (lane & 31);
      const unsigned want = hs_tag(R.seq, lane < 32 ? tl : prow);
      unsigned long long v = 0;
      bool ok = !(mine || theirs);
      int spins = 0, bad = 0;
      for (;;) {
        if (!ok) {
          v = multi ? hs_ld_sys(src) : hs_ld_sc1(src);
          ok = (unsigned)(v >> 32) == want;
        }
        if (__builtin_amdgcn_ballot_w64(ok) == ~0ull) break;
        if (HSR_A_AHEAD) HSR_A_NOT_YET;  // (not there yet: this walker's turn will wait for them)
        ++spins;
        if ((spins & 255) == 0) {  // somebody else has given up: so do we
          int st = 0;
          if (lane == 0)
            st = (int)__hip_atomic_load(R.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          st = __builtin_amdgcn_readfirstlane(st);
          if (st != 0) { bad = HS_RUN_ERR_PEER; break; }
        }
        if (spins > R.spin_limit) { bad = HS_RUN_ERR_TIMEOUT; break; }
        __builtin_amdgcn_s_sleep(1);
      }
      slice_bad = bad;
      if (bad) {
        if (lane == 0) {
          hi[HI_TICK] = bad;
          if (bad == HS_RUN_ERR_TIMEOUT)
            __hip_atomic_store(R.status, bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      const unsigned pl = (unsigned)v;
      const int d2 = (2 * lane) & 31;
      const unsigned mlo = (unsigned)__shfl((int)pl, d2, 64);
      const unsigned mhi = (unsigned)__shfl((int)pl, d2 + 1, 64);
      const unsigned plo = (unsigned)__shfl((int)pl, 32 + d2, 64);
      const unsigned phi = (unsigned)__shfl((int)pl, 33 + d2, 64);
      const double sme = __hiloint2double((int)mhi, (int)mlo);
      const double spa = __hiloint2double((int)phi, (int)plo);
      const double q = spa - (spa - sme) * mz;  // emcee StretchMove.get_proposal
      if (lane < ndim) {
        qs[lane] = q;
        olds[lane] = sme;
      }
      if (lane == ndim) accs[2] = sme;  // the old log-probability rides behind the coordinates
      if (lane == 0) {
        accs[0] = mz;
        accs[1] = mlnu;
        hi[HI_ME] = me;
        hi[HI_PA] = pa;
      }
      if (!(HSR_A_AHEAD)) HSR_STAMP(1);
      // the packs: thread t < 8 npacks evaluates column t % 8 of pack t / 8 from ONE proposed
      // coordinate (which one is walker-independent: a byte of pkd), taken by a shuffle
      const double qv = __shfl(q, pkd < 0 ? 0 : pkd, 64);
      if (lane < npk8) {
        const double za = pk_a, zb = pk_b, zc = pk_c;
        const int ztf = pk_tf, nc = pk_nc;
        const int col = lane % NH_MAX_LAZY;
        if (col < nc) {
          double val = za;
          // (the common fit -- every column the identity or a power of ten of its coordinate: one
          // exp10 for the wave and a select.  hsr_lazy_apply takes the transform in a vector register
          // and walks its switch as exec-mask regions, case by case: ~40 vector instructions of
          // compares and masks around the 45 of the one transform that is there, on the wave
          // everybody waits for.  The same operations on the same operands: the same bits.)
          const bool odd = pkd >= 0 && ztf != NH_TF_ID && ztf != NH_TF_POW10;
          if (__builtin_amdgcn_ballot_w64(odd) == 0ull) {
            const double xl = zb * qv + zc;
            const double xe = hsr_exp10(xl);
            if (pkd >= 0) val = za * (ztf == NH_TF_POW10 ? xe : xl);
          } else if (pkd >= 0) {
            val = hsr_lazy_apply(za, zb, zc, ztf, qv);
          }

          if (lane / NH_MAX_LAZY == H.F.ppk) {  // the particle rows: also into LDS
            row[col] = val;
            // (ln of e_0, e_cutoff, e_break for the weights; ln |amplitude| and its sign for the
            // log-domain synchrotron items.  A constant's logarithm was taken when the launch
            // began; a power of ten -- naima's fits walk in log10 of the amplitude and of the
            // energies -- has ln|a 10^y| = ln|a| + y ln 10 in two FMAs, as good as the logarithm of
            // the rounded power (both are right to the last place of a number around 70); only
            // another transform calls the library's log behind its own result -- the chain
            // exp10 -> log on one lane was 0.4 us of every slice with every other wave waiting)
            // (ln |amplitude|: only the log-domain synchrotron items read it -- for a table-only
            // model whose amplitude is not a power of ten, cfg1's, it was a library log on the one
            // wave everybody waits for)
            if (((SYN && S2) && col == 0) || col == 1 || col == 3 || col == 5) {
              double lv;
              const bool easy = pkd < 0 || ztf == NH_TF_POW10;
              if (pkd < 0) {
                lv = pk_lna;
              } else if (ztf == NH_TF_POW10) {
                lv = hs_ln_pow10(pk_lna, zb, zc, qv);
              } else {
                lv = 0.0;
              }
              if (__builtin_amdgcn_ballot_w64(!easy) != 0ull) {
                asm volatile("" ::: "memory");  // (keep the call behind the branch)
                const double lv2 = hsr_log(fabs(val));
                lv = easy ? lv : lv2;
              }
              if (col == 0) {
                qs[HS_O_LNA] = lv;
                qs[HS_O_LNA + 1] = val < 0.0 ? -1.0 : 1.0;
              } else {
                lg[col >> 1] = val > 0.0 ? lv : pk_ln0;
              }
            }
          }
          pval = val;
          pcol = col;
        }
      }
