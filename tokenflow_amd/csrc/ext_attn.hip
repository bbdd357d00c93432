// Extended (cross-keyframe) attention forward for gfx950.
// Replaces tokenflow_utils.py:124-197 / 234-279 of omerbt/TokenFlow: the per-head
// bmm -> *scale -> softmax -> bmm loops over a K-times replicated key/value bank.
//
// Flash-style: one workgroup = 128..256 queries of one (branch, frame, head); it streams the
// key/value sequence (S keys for the source branch, the K*S-key bank of the branch for
// uncond / cond) in 64-key tiles with an online softmax; nothing of size S x K*S exists.
// q/k are read in place from the [3,K,S,H*Dh] projection output (head = a Dh-wide column
// slab, token stride ld); PnP injection is pointer aliasing of the source branch's q/k.
//
// MFMA mapping (v_mfma_f32_32x32x16, 64-lane waves, one wave = 32 queries):
//   S^T = K . Q^T   A = K tile rows (keys) from LDS, B = Q fragments held in registers
//                   -> lane owns ONE query (col = lane & 31) and 16 keys per 32-key tile:
//                      softmax statistics are lane-local (+1 exchange with lane ^ 32).
//   O^T = V^T . P   A = V^T rows (d) from LDS, B = P straight from the S^T accumulator
//                   registers: C/D register r of lane half hi is key (r&3)+8(r>>2)+4hi, so
//                   regs 0..7 / 8..15 are the two 16-key k-steps.  The V^T image stores keys
//                   in exactly that order (bits 2 and 3 of the key index swapped inside
//                   every 16-key group), so P needs NO cross-lane movement at all.
//   The alpha rescale of O^T is lane-local as well (col = query).
// V^T comes from a small pre-pass (vt_pack_kernel) that writes the bank transposed,
// key-permuted and zero-padded per frame to a multiple of 128 keys into caller-provided scratch
// (1 read + 1 write of V, ~1.4% of the attention time at the sizes that matter).
// LDS: double-buffered K [64][DKP+8] and V^T [32*MT][64+8] tiles; the +8 element pad makes
// every row stride an odd number of 16-B slots -> conflict-free ds_read_b128.
// Pipeline: tile i+1 is fetched global->registers before the MFMAs of tile i and written
// to the other LDS buffer after them; one barrier per tile.
// Block order: head = blockIdx % H, so with H = 8 every XCD (block b runs on XCD b % 8)
// serves one head and its L2 holds only that head's bank; bank problems are queued
// before the short source problems so the tail of the grid is filled with short work.
// Three kernels share this structure (geometry table and measurements: DESIGN.md section 4.1):
//   ext_attn_kernel<.., MODE_ALL / MODE_SOURCE>  the plain form
//   ext_attn_kernel<.., MODE_DUAL>               q/k injection: uncond + cond share QK^T and the softmax
//   ext_attn_pp_kernel                           two query tiles per wave, softmax of one interleaved
//                                                in program order with the MFMAs of the other
//   ext_attn_il_kernel                           one query tile per wave pipelined over 32-key half tiles (attn_il.h)
//
// Files: attn_common.h (parameter blocks, tile geometry, helpers), attn_prepost.h (vt_pack_kernel, the merge kernels),
// attn_plain.h / attn_pp.h / attn_il.h (one streaming kernel each, with its schedule and its launch_*); this file keeps the
// split plan, the dispatcher, the workspace arithmetic and the entry points.  One translation unit.
#include "attn_common.h"
#include "attn_il.h"
#include "attn_plain.h"
#include "attn_pp.h"
#include "attn_prepost.h"

namespace {

// How many runs of bank frames a bank problem is split into.  The grid of a sharded rank or of a small level has
// too few waves to fill the chip (8-GPU rank at cfg2 level 0: 2 waves per SIMD, level 1: 0.5; single GPU at the
// 16x16 level: 1): split until it has `occ` waves per SIMD, while a run keeps at least 2 tiles.
static int split_plan(int K, int Kq, int S, int H, int Dh, bool inject, int part, bool allow) {
    if (!allow || part == TF_ATTN_SOURCE_ONLY) return 1;
    const bool dual = inject && S >= 256 && Dh != 160;
    // Dh = 160: splitting towards 2 waves per SIMD (the single-buffered tiles would allow two workgroups per CU) measured
    // slower: 88 vs 85 us at cfg2 level 2, 41 vs 33 us on a rank of 8 (merge included)
    constexpr int OCC160 = 1;
    const int occ = Dh == 40 ? 4 : Dh == 160 ? OCC160 : dual ? 2 : Dh == 64 ? 4 : 3;   // waves per SIMD the kernels reach
    const int64_t wgs = (int64_t)(dual ? 1 : 2) * Kq * ((S + 127) / 128) * H;   // 4-wave workgroups
    const int tpf = (S + 63) / 64;
    if (K * tpf < 16) return 1;   // a bank of a few tiles: the merge launch costs more than it buys (8x8 level)
    int nseg = 1;
    while (wgs * 4 * nseg < (int64_t)occ * 1024 && nseg * 2 <= K && (K / (nseg * 2)) * tpf >= 2) nseg *= 2;
    // A SHORT bank (<= 8192 keys) that already has half the waves the kernel can hold gains less from the second half than the
    // partial results + merge launch cost: BASELINE config 1, level 0 (K = 4, S = 1024, 2 of 4 waves per SIMD): 0.091 against
    // 0.098 ms unsplit (round 6, one box, TOKENFLOW_ATTN_NSEG A/B); the dual-V launch keeps its split (0.092 against 0.111)
    if (!dual && nseg == 2 && (int64_t)K * S <= 8192) nseg = 1;
    // TOKENFLOW_ATTN_NSEG=n (experiments): force n runs
    static const int forced = [] { const char* e = getenv("TOKENFLOW_ATTN_NSEG"); return e ? atoi(e) : 0; }();
    if (forced > 0) return forced <= K ? forced : K;
    // Large grids: splitting every bank problem into n runs of frames so that the last, nearly empty round of workgroups gets
    // shorter (cfg4 level 0: 3600 bank workgroups on 512 resident slots = 7.03 rounds) was modelled and measured in round 6
    // (profiles/r06_attn_tail_split.txt): n = 2 gains 1.7 % at cfg4 level 0 and 3 % at its level 1, costs 5 % at cfg5 level 0
    // and 3 % at cfg2 level 0; n = 5 loses everywhere (+5..14 %).  The rounds are not in lockstep, the source problems fill
    // the tail, and the partial results' round trip costs more than the model allowed: no planner, the switch above stays.
    // TOKENFLOW_SPLIT_OVER=n (experiments): n further doublings once the chip is full -- shorter workgroups, so that a
    // launch running BESIDE this one (a rank's source branch on an auxiliary stream) is absorbed instead of appended
    static const int over = [] { const char* e = getenv("TOKENFLOW_SPLIT_OVER"); return e ? atoi(e) : 0; }();
    for (int i = 0; i < over && nseg > 1 && nseg * 2 <= K && (K / (nseg * 2)) * tpf >= 2; ++i) nseg *= 2;
    return nseg;
}

// Geometry per head dim (A/B-measured on MI355X, tools/attn_microbench.py): what matters is the number of
// INDEPENDENT waves per SIMD (softmax VALU of one wave overlaps MFMAs of another) and how many waves share
// one staged tile.  Dh=40: 1 query tile/wave, 8 waves/workgroup, 111 VGPRs -> 4 waves/SIMD.
// Dh=64: 2 query tiles/wave (each LDS fragment feeds 2 MFMAs).  Dh=80/160: register-bound, 1 tile/wave.
template <typename T, int DH, typename P>
int launch_attn(const P& p, const void* v, hipStream_t st) {
    constexpr bool WIN = is_win<P> || is_set<P>;   // windowed / frame-set call: no run or folded-scale form (refused by the entry points)
    const bool src_only = p.part == TF_ATTN_SOURCE_ONLY, bank_only = p.part == TF_ATTN_BANK_ONLY;
    // The kernel FAMILY of a run launch is the one the unsplit call of the same (Kq, S, H) takes, however the run splits
    // itself: the source branch out of a run call is then bit for bit the source-only call's (same kernel, same keys).
    const int ns_sel = p.run ? 1 : p.nseg;
    if (!p.no_pack) {   // pre-pass: V -> transposed, key-permuted, per-frame padded bank (only the branches this call computes)
        // (a run launch: the run's p.K frames only, at their positions in the image of the whole bank -- p.vt, p.knorm2, p.k and v
        // point at the run's first frame, so the runs of one bank fill disjoint parts of one workspace)
        // key norms: of every branch's own keys; under injection of the source's, by the first packed branch
        const int b_lo = bank_only ? 1 : 0;
        if (const int rc = launch_vt_pack<T>(p, v, DH, b_lo, src_only ? 1 : 3, p.inject ? 0u : ~0u, p.inject ? b_lo : -1, st))
            return rc;
    }
    // Every head dim has three forms: ALL (one launch, bank problems then source problems), DUAL (injection:
    // uncond + cond share QK^T and the softmax; pays from S = 256 on) and SOURCE (the source branch alone).
    // A full call is ALL, or DUAL followed by SOURCE; a bank-only call drops the source part, a source-only
    // call is SOURCE alone.
    auto merge = [&]() -> int {   // split form: fold the per-run partial results into the output
        if (p.nseg <= 1 || p.run) return 0;   // (a run's partial results wait for tf_ext_attn_runs_merge)
        if (tf_plan_note("merge[nseg=%d]", p.nseg)) return 0;
        const int64_t total = (int64_t)2 * p.Kq * p.H * p.S * (DH / 4);
        const int64_t blocks = (total + 255) / 256;
        hipLaunchKernelGGL(attn_merge_kernel<T>, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st,
                           p.partials, p.out, p.Kq, p.S, p.H, DH, p.nseg, p.out_f32, p.o_bs, p.o_fs);
        TF_LAUNCH_CHECK("tf_ext_attn_fwd(merge)");
        return 0;
    };
    auto compose = [&](auto all, auto dual, auto source) -> int {
        if (src_only) return source();
        if (!p.inject || (p.S < 256 && !p.force_dual)) {   // short frames: the ALL form reads the source q, k itself
            const int rc = all();
            return rc ? rc : merge();
        }
        int rc = dual();
        if (!rc) rc = merge();
        return (rc || bank_only) ? rc : source();
    };
    if constexpr (DH == 40) {
        // 8-wave (256-query) workgroups while they still give 3 workgroups per CU (split runs included: measured
        // -8..11 % on a sharded rank's level 0 against the 4-wave form); below that the 4-wave form (twice the
        // workgroups).  S < 256: always 4 waves.
        const bool big = p.S >= 256 && (int64_t)3 * p.Kq * ((p.S + 255) / 256) * p.H * ns_sel >= 768;
        // multi-edit batch under injection: two edits' bank branches in one launch (tf_ext_attn_fwd_edits), 4-wave workgroups,
        // two per CU (70 KB of tiles each)
        if (p.mv4) return launch_one<T, DH, 4, MODE_MV4, 2, false>(p, st);
        if (!p.fold || WIN) {   // fp32 score scaling: the default (a windowed call has no other: TF_ATTN_FOLD_SCALE is refused)
            // one 8-wave workgroup per CU: a W = 8 rank's one-pass level 0 (384 workgroups) runs
            // 586 us interleaved against 672 us in the plain 4-wave form (profiles/r03_rank_shard.txt)
            constexpr int IL40_MIN_WGS = 256;
            // half-tile interleaved form (ext_attn_il_kernel); TF_ATTN_HINT_MIX (p.mix) opens it on any grid its shape
            // requirement admits, so that the mixed-shape form it selects below is taken whatever the launch size
            const bool il = p.S >= 256 && p.S % 64 == 0 &&
                            (p.mix || (int64_t)3 * p.Kq * ((p.S + 255) / 256) * p.H * ns_sel >= IL40_MIN_WGS);
            // Round 6: K / V^T tiles by LDS-DMA into the padded images (117 instead of 128 VGPRs, no ds_write pass, fragment
            // addresses unchanged): 3.57 against 3.64 ms at cfg2 level 0 (profiles/r06_attn_d40_ab.txt).
            constexpr int IL40_NW = 8, IL40_MINW = 4, IL40_DMA = 2;   // waves per workgroup, min waves per SIMD, staging
            // Round 6, last session: mixed MFMA shapes (DMA = 3: QK^T 32x32x16, P.V 16x16x32 over 16-row M-tiles, see IlScheduleMix) --
            // level-0 launch 3.57 -> 3.43 ms, cfg2 step 25.04 -> 24.48 ms on one box (profiles/r06_attn_d40_mix_ab.txt).  Its softmax is
            // placed by hipcc, in coarser alternation with the MFMAs than the pinned steps: launches of ONE round of workgroups, whose
            // waves run in lockstep, lose with it (a rank of 8, level 0: 3.96-4.01 against 3.88-3.89 ms per rank step, section 9 of the
            // same file) -> only launches of >= 2 rounds (1024 eight-wave workgroups), and never in the bit-stable mode, whose kernel
            // choice must be a function of the shape alone (a rank and the single GPU must agree bit for bit there).
            constexpr int IL40_MIX_MIN_WGS = 1024;
            const int64_t per_branch = (int64_t)p.Kq * ((p.S + 255) / 256) * p.H;
            const bool mix_all = p.mix || (!p.bit_stable && per_branch * (2 * ns_sel + (bank_only ? 0 : 1)) >= IL40_MIX_MIN_WGS);
            const bool mix_src = p.mix || (!p.bit_stable && per_branch >= IL40_MIX_MIN_WGS);
            if (il)
                return compose([&] { return mix_all ? launch_il<T, 40, IL40_NW, MODE_ALL, IL40_MINW, 3>(p, st)
                                                    : launch_il<T, 40, IL40_NW, MODE_ALL, IL40_MINW, IL40_DMA>(p, st); },
                               [&] {
                                   // Round 6: the packed dual-V kernel with LDS-DMA staging, 8-wave workgroups, FOUR waves per SIMD (128
                                   // VGPRs; the register-staged 4-wave form needs 168 = 3 per SIMD): 2.54 against 2.81 ms at cfg2 level 0
                                   // (profiles/r06_attn_d40_dual_ab.txt; DMA alone at 3 waves per SIMD: 2.70)
                                   constexpr int IL40_DUAL_NW = 8, IL40_DUAL_MINW = 4, IL40_DUAL_DMA = 2;
                                   if (p.S >= 256 && p.S % 64 == 0)
                                       return launch_il<T, 40, IL40_DUAL_NW, MODE_DUAL, IL40_DUAL_MINW, IL40_DUAL_DMA>(p, st);
                                   return launch_one<T, DH, 4, MODE_DUAL, 3, false>(p, st);
                               },
                               [&] { return mix_src ? launch_il<T, 40, IL40_NW, MODE_SOURCE, IL40_MINW, 3>(p, st)
                                                    : launch_il<T, 40, IL40_NW, MODE_SOURCE, IL40_MINW, IL40_DMA>(p, st); });
            // grids too small for the interleaved form, ragged or short frames: the plain kernel.  (Source-only grids below 256
            // 8-wave workgroups as 4-wave workgroups measured slower, profiles/r05_rank_step_src4_ab.txt.)
            return compose([&] { return big ? launch_one<T, DH, 8, MODE_ALL, 2, false>(p, st)
                                            : launch_one<T, DH, 4, MODE_ALL, 2, false>(p, st); },
                           [&] {
                               // (the register-staged 4-wave interleaved dual-V form: the only DMA = 0 launch)
                               if (p.S >= 256 && p.S % 64 == 0) return launch_il<T, 40, 4, MODE_DUAL, 3, 0>(p, st);
                               return launch_one<T, DH, 4, MODE_DUAL, 3, false>(p, st);
                           },
                           [&] { return big ? launch_one<T, DH, 8, MODE_SOURCE, 2, false>(p, st)
                                            : launch_one<T, DH, 4, MODE_SOURCE, 2, false>(p, st); });
        }
        if constexpr (WIN)
            return TF_ERR_SHAPE;   // never reached (tf_ext_attn_fwd_windows refuses the folded scale): keeps the folded-scale
                                   // kernels from being instantiated on the windowed parameter block
        else
            return compose([&] { return big ? launch_one<T, DH, 8, MODE_ALL, 2>(p, st)
                                            : launch_one<T, DH, 4, MODE_ALL, 2>(p, st); },
                           [&] { return launch_one<T, DH, 4, MODE_DUAL, 3>(p, st); },   // 151 VGPRs: 3 workgroups per CU
                           [&] { return big ? launch_one<T, DH, 8, MODE_SOURCE, 2>(p, st)
                                            : launch_one<T, DH, 4, MODE_SOURCE, 2>(p, st); });
    } else if constexpr (DH == 64) {
        // Round 6: the half-tile interleaved kernel with its K / V^T tiles staged by LDS-DMA into the padded images (no staging
        // registers: 124 VGPRs, FOUR waves per SIMD) and the score bound -- 1067 / 1082 TF/s at cfg4 / cfg5 level 0 against
        // 971 / 982 of the ping-pong kernel on the same box (profiles/r06_attn_d64_ab.txt; the register-staged interleaved form
        // of round 5 needed 136 VGPRs = 3 waves per SIMD and lost to it).  The mixed MFMA shapes measured 6 % slower here
        // (profiles/r06_attn_d64_mix_ab.txt).
        constexpr int IL64_NW = 8, IL64_MINW = 4, IL64_DMA = 2;   // waves per workgroup, min waves per SIMD, staging
        // multi-edit batch under injection: two edits' bank branches in one launch (tf_ext_attn_fwd_edits, TF_ATTN_MULTI_V64).
        // Four unpacked 64-row banks, 92 KB of double-buffered tiles: ONE workgroup per CU, so 8 waves for two per SIMD (246 VGPRs)
        if (p.mv4) return launch_one<T, DH, 8, MODE_MV4, 2>(p, st);
        const bool il = p.S % 64 == 0 && p.S >= 512;
        // A run through the ping-pong kernel: its bank problems in the partial form, then the source branch through the kernel
        // the source-only call takes (the ping-pong kernel's own source problems are a different arithmetic)
        auto run_pp = [&]() -> int {
            AttnParams pb = p;   // (never a windowed call: those are no runs)
            pb.part = TF_ATTN_BANK_ONLY;
            const int rc = launch_pp<T, true>(pb, st);
            return (rc || bank_only) ? rc : launch_one<T, DH, 4, MODE_SOURCE, 2>(p, st);
        };
        return compose([&] { return il ? launch_il<T, DH, IL64_NW, MODE_ALL, IL64_MINW, IL64_DMA>(p, st)
                                  : (p.S >= 512 && p.nseg == 1 && p.run) ? run_pp()
                                  : (p.S >= 512 && p.nseg == 1) ? launch_pp<T>(p, st)   // ragged frames: ping-pong
                                                                : launch_one<T, DH, 4, MODE_ALL, 2>(p, st); },
                       [&] {
                                // Round 6: q/k injection in the interleaved kernel too -- both V banks in one 4-M-tile image (uncond rows
                                // 0-63, cond 64-127), 12 MFMAs per phase against the same 8 softmax units, 162 VGPRs, 2 workgroups of 4 waves
                                // per CU: 18.99 against 20.27 ms at cfg4 level 0, 2.47 / 2.61 at level 1, 0.359 / 0.380 at level 2
                                // (profiles/r06_attn_d64_dual_ab.txt; 8-wave workgroups: 2.35 ms at level 1 but 0.46 at level 2)
                                constexpr int IL64_DUAL_NW = 4;
                                if (il) return launch_il<T, DH, IL64_DUAL_NW, MODE_DUAL, 2, 2>(p, st);
                                return launch_one<T, DH, 4, MODE_DUAL, 2>(p, st); },
                       [&] { return il ? launch_il<T, DH, IL64_NW, MODE_SOURCE, IL64_MINW, IL64_DMA>(p, st)
                                       : launch_one<T, DH, 4, MODE_SOURCE, 2>(p, st); });
    } else if constexpr (DH == 80) {
        // Round 6: LDS-DMA staging (padded images) frees the staging registers: 146 VGPRs with 4-wave workgroups, THREE of which
        // fit a CU (3 waves per SIMD, 3 x 50 KB of LDS) -- 0.442 against 0.482 ms at cfg2 level 1 (profiles/r06_attn_d80_ab.txt;
        // register-staged: 8 waves, 166 VGPRs, 2 waves per SIMD; DMA with 8-wave workgroups: no change, 0.479)
        constexpr int IL80_NW = 4, IL80_MINW = 3, IL80_DMA = 2;   // waves per workgroup, min waves per SIMD, staging
        const bool il = p.S % 64 == 0 && p.S >= 256;   // half-tile interleaved form (ext_attn_il_kernel)
        return compose([&] { return il ? launch_il<T, DH, IL80_NW, MODE_ALL, IL80_MINW, IL80_DMA>(p, st)
                                       : launch_one<T, DH, 4, MODE_ALL, 2>(p, st); },
                       [&] {
                                // Round 6: q/k injection in the interleaved kernel at d = 80 too -- both V banks in one 5-M-tile image
                                // (uncond rows 0-79, cond 80-159), 184 VGPRs, 2 workgroups of 4 waves per CU: 0.332-0.344 against
                                // 0.374 ms at cfg2 level 1 on one box (profiles/r06_attn_d80_dual_ab.txt)
                                if (il) return launch_il<T, DH, 4, MODE_DUAL, 2, 2>(p, st);
                                return launch_one<T, DH, 4, MODE_DUAL, 2>(p, st); },
                       [&] { return il ? launch_il<T, DH, IL80_NW, MODE_SOURCE, IL80_MINW, IL80_DMA>(p, st)
                                       : launch_one<T, DH, 4, MODE_SOURCE, 2>(p, st); });
    } else {
        // Dh=160: the dual (shared-softmax) form needs 160 more accumulator registers and measured slower;
        // under injection the ALL form reads the source q and k for every branch instead.  The interleaved kernel
        // was measured here too (8 waves sharing the 89 KB of tiles, 237 VGPRs): 97 vs 92 us at cfg2 level 2 -- at
        // this head dim every MFMA needs its own 1 KB fragment from LDS, whose read rate (128 B/clk per CU) equals
        // the matrix pipes' demand, and the level has one wave per SIMD whatever the kernel.
        // single LDS buffer: 44.5 instead of 89 KB per workgroup.  85 vs 95 us at cfg2 level 2 (profiles/r03_attn_sb160.txt):
        // at one wave per SIMD the second buffer bought no overlap, and two workgroups now fit a CU where the grid has them
        if (src_only) return launch_one<T, DH, 4, MODE_SOURCE, 1, true, true>(p, st);
        const int rc = launch_one<T, DH, 4, MODE_ALL, 1, true, true>(p, st);
        return rc ? rc : merge();
    }
}

template <typename T, typename P>
int dispatch_dh(int Dh, const P& p, const void* v, hipStream_t st) {
    switch (Dh) {
        case 40: return launch_attn<T, 40>(p, v, st);
        case 64: return launch_attn<T, 64>(p, v, st);
        case 80: return launch_attn<T, 80>(p, v, st);
        case 160: return launch_attn<T, 160>(p, v, st);
    }
    return TF_ERR_SHAPE;
}

}  // namespace

// Workspace of a call over `branches` branches: V^T image | key norm bounds | split-form partial results (of one edit: the
// edits of a multi-edit batch run one behind the other on the stream and reuse them)
static size_t attn_part_elems(int K, int S, int H, int Dh) {
    size_t part_elems = 0;   // split form: worst case over the number of query frames a caller may pass
    for (int Kq = 1; Kq <= K; ++Kq)
        for (int inj = 0; inj < 2; ++inj) {
            const int ns = split_plan(K, Kq, S, H, Dh, inj != 0, 0, true);
            const size_t e = ns > 1 ? (size_t)2 * Kq * H * S * ns * (Dh + 8) : 0;
            part_elems = e > part_elems ? e : part_elems;
        }
    return part_elems;
}

static size_t attn_ws_bytes(int K, int S, int H, int Dh, int dtype, int branches) {
    if (K <= 0 || S <= 0 || H <= 0 || Dh <= 0 || dtype == TF_F32) return 0;
    const size_t Spad = (size_t)((S + 127) / 128) * 128;   // frames padded to the largest staged tile
    return ((vt_bytes(K, (int)Spad, H, Dh, branches) + 255) & ~(size_t)255) +
           (((size_t)branches * H * K * (Spad / 64) * sizeof(float) + 255) & ~(size_t)255) +
           attn_part_elems(K, S, H, Dh) * sizeof(float);   // V^T image | key norm bounds | split-form partial results
}

// Workspace of a pass of keyframe segments (tf_ext_attn_fwd_segments): the image and the norm table of the whole bank of K
// frames; the split-form partial results of the largest segment's own call (the segments run one behind the other on the stream
// and reuse them), whatever the segmentation: the worst case over every bank size up to K
static size_t attn_seg_ws_bytes(int K, int S, int H, int Dh, int dtype) {
    if (K <= 0 || S <= 0 || H <= 0 || Dh <= 0 || dtype == TF_F32) return 0;
    const size_t Spad = (size_t)((S + 127) / 128) * 128;
    size_t part_elems = 0;
    for (int Kv = 1; Kv <= K; ++Kv) {
        const size_t e = attn_part_elems(Kv, S, H, Dh);
        part_elems = e > part_elems ? e : part_elems;
    }
    return ((vt_bytes(K, (int)Spad, H, Dh, 3) + 255) & ~(size_t)255) +
           (((size_t)3 * H * K * (Spad / 64) * sizeof(float) + 255) & ~(size_t)255) + part_elems * sizeof(float);
}

extern "C" size_t tf_ext_attn_workspace_bytes(int K, int S, int H, int Dh, int dtype) {
    return attn_ws_bytes(K, S, H, Dh, dtype, 3);
}

namespace {

// One part of a multi-edit batch (tf_ext_attn_fwd_edits) as seen by the single-edit call that computes it: the caller has
// moved the base pointers of q / k / v / out to the edit's slabs; the workspace holds the image of all `branches` branches
// and the launches read it `shift` branches in (2 per edit in front of this one).
struct EditsPart {
    int branches;   // 1 + 2E
    int shift;      // branches in front of this edit's uncond branch, minus 1: 2 * edit
    int no_pack;    // the V^T pre-pass has been issued for all branches
    int mv4;        // this call computes TWO edits' bank branches in the four-bank form
    int gap;        // ... whose uncond branches lie `gap` branches apart (2 = neighbouring edits)
    int force_dual; // the DUAL launch at any S
    int probe;      // do not launch: return 1 if the call takes the fused small-problem kernel, else 0

    // the parts of a batch of `branches` branches whose V^T image is packed: edit e's bank branches through the launches of
    // its own bank-only call / the pair (e0, e1), e0 < e1, in the four-bank form / edit e in the DUAL launch at any S / the
    // source branch / the probe of a part's fused-kernel decision
    static EditsPart bank(int branches, int e) { return make(branches, 2 * e, 0, 0, 0); }
    static EditsPart pair_mv4(int branches, int e0, int e1) {
        EditsPart p = make(branches, 2 * e0, 1, 0, 0);
        p.gap = 2 * (e1 - e0);
        return p;
    }
    static EditsPart bank_dual(int branches, int e) { return make(branches, 2 * e, 0, 1, 0); }
    static EditsPart source(int branches) { return make(branches, 0, 0, 0, 0); }
    static EditsPart probe_of(int branches) { return make(branches, 0, 0, 0, 1); }

private:
    static EditsPart make(int branches, int shift, int mv4, int force_dual, int probe) {
        EditsPart p{};
        p.branches = branches, p.shift = shift, p.no_pack = 1, p.mv4 = mv4, p.force_dual = force_dual, p.probe = probe;
        p.gap = 2;
        return p;
    }
};

// One keyframe segment of a pass (tf_ext_attn_fwd_segments) as seen by the single-clip call that computes it: the caller has
// moved the base pointers of q / k / v / out to the segment's first frame and packed the V^T image of the WHOLE bank of
// `K_all` frames; K = Kq = the segment's frames, and the launches read the image and the norm table from frame `f0` on with
// the whole bank's row strides (p.Kb), the way a run call folds its frame window.
struct SegPart {
    int K_all;
    int f0;
    int probe;   // do not launch: return 1 if the segment's own call takes the fused small-problem kernel, else 0
};

// A call over a sliding-window bank (tf_ext_attn_fwd_windows): the validated table, packed as the kernels read it, and the
// longest window -- the bank size at which the call picks its kernel forms.
struct WinPart {
    const unsigned* win;   // [Kq]: first bank frame | frames << 16
    int K_max;
};

// A call over a frame-set bank (tf_ext_attn_fwd_frame_sets): the validated member masks and the largest set -- the bank size at
// which the call picks its kernel forms.
struct SetPart {
    const uint64_t* set;   // [Kq]: bit j = bank frame j is a member
    int K_max;
};

int attn_fwd_core(const void* q, const void* k, const void* v, void* out, int K, int Kq, int q_frame0, int S, int H, int Dh,
                  int64_t ld, const int64_t* strides, float scale, int inject, int dtype, void* ws, size_t ws_bytes,
                  void* stream, const EditsPart* ed, const SegPart* sg = nullptr, const WinPart* wn = nullptr,
                  const SetPart* fs = nullptr) {
    const int K_plan = wn ? wn->K_max : fs ? fs->K_max : K;   // windows / frame sets: planned for the longest window / largest set
    TF_ARG(q && k && v && out && ws && strides, TF_ERR_NULL, "tf_ext_attn_fwd: null pointer");
    TF_ARG(dtype == TF_BF16 || dtype == TF_F16, TF_ERR_DTYPE, "tf_ext_attn_fwd: dtype %d (bf16/f16 only)", dtype);
    TF_ARG(Dh == 40 || Dh == 64 || Dh == 80 || Dh == 160, TF_ERR_SHAPE,
           "tf_ext_attn_fwd: head dim %d not in {40,64,80,160}", Dh);
    TF_ARG(K > 0 && S > 0 && H > 0 && ld >= (int64_t)H * Dh && ld % 8 == 0, TF_ERR_SHAPE,
           "tf_ext_attn_fwd: K=%d S=%d H=%d ld=%lld (ld a multiple of 8, >= H*Dh)", K, S, H, (long long)ld);
    TF_ARG(Kq > 0 && q_frame0 >= 0 && q_frame0 + Kq <= K, TF_ERR_SHAPE,
           "tf_ext_attn_fwd: query frames [%d, %d) outside the %d-frame bank", q_frame0, q_frame0 + Kq, K);
    const int64_t ld_q = strides[8];
    TF_ARG(ld_q >= (int64_t)H * Dh && ld_q % 8 == 0, TF_ERR_SHAPE,
           "tf_ext_attn_fwd: q token stride %lld (a multiple of 8, >= H*Dh)", (long long)ld_q);
    for (int i = 0; i < 8; ++i)
        TF_ARG(strides[i] % 8 == 0 &&
                   (i & 1 ? strides[i] >= (int64_t)(S - 1) * (i < 2 ? ld_q : i < 6 ? ld : (int64_t)H * Dh) : true),
               TF_ERR_SHAPE, "tf_ext_attn_fwd: stride %d = %lld (multiples of 8 elements; a frame holds S token rows)", i,
               (long long)strides[i]);
    TF_ARG(tf_aligned16(q) && tf_aligned16(k) && tf_aligned16(v) && tf_aligned16(out) && tf_aligned16(ws),
           TF_ERR_ALIGN, "tf_ext_attn_fwd: tensors not 16-byte aligned");
    const int branches = ed ? ed->branches : 3;
    const size_t ws_need = sg ? attn_seg_ws_bytes(sg->K_all, S, H, Dh, dtype) : attn_ws_bytes(K, S, H, Dh, dtype, branches);
    TF_ARG(ws_bytes >= ws_need, TF_ERR_WORKSPACE, "tf_ext_attn_fwd: workspace %zu < %zu bytes", ws_bytes, ws_need);
    const int part_bits = inject & (TF_ATTN_BANK_ONLY | TF_ATTN_SOURCE_ONLY);
    TF_ARG(part_bits != (TF_ATTN_BANK_ONLY | TF_ATTN_SOURCE_ONLY), TF_ERR_SHAPE,
           "tf_ext_attn_fwd: TF_ATTN_BANK_ONLY and TF_ATTN_SOURCE_ONLY exclude each other");
    {   // small problems: one fused launch, no pre-pass, no merge (csrc/ext_attn_fused.hip)
        TfAttnSet a{};
        a.q = q, a.k = k, a.v = v, a.out = out;
        a.q_bs = strides[0], a.q_fs = strides[1], a.ld_q = ld_q;
        a.k_bs = strides[2], a.k_fs = strides[3], a.v_bs = strides[4], a.v_fs = strides[5], a.ld = ld;
        a.o_bs = strides[6], a.o_fs = strides[7];
        a.H = H, a.Kq = Kq, a.q_frame0 = q_frame0, a.Kb = K_plan;
        a.b0 = part_bits == TF_ATTN_BANK_ONLY ? 1 : 0;
        a.nb = part_bits == TF_ATTN_BANK_ONLY ? 2 : part_bits == TF_ATTN_SOURCE_ONLY ? 1 : 3;
        const TfFusedPlan plan = tf_attn_fused_plan(&a, 1, S, Dh, dtype, inject);
        if ((ed && ed->probe) || (sg && sg->probe)) return plan.use ? 1 : 0;
        a.Kb = K;
        if (plan.use)
            return tf_attn_fused_launch(&a, 1, S, Dh, scale, inject, dtype, plan, reinterpret_cast<hipStream_t>(stream),
                                        wn ? wn->win : nullptr, fs ? fs->set : nullptr);
    }
    const int Spad = ((S + 127) / 128) * 128;
    const int shift = ed ? ed->shift : 0;
    const int Kb = sg ? sg->K_all : K;   // frames of the image and of the norm table
    const size_t vt_all = (vt_bytes(Kb, Spad, H, Dh, branches) + 255) & ~(size_t)255;
    const size_t kn_all = ((size_t)branches * H * Kb * (Spad / 64) * sizeof(float) + 255) & ~(size_t)255;
    unsigned char* const w8 = static_cast<unsigned char*>(ws);
    AttnParams p{};
    p.q = q;
    p.k = k;
    p.inject = (inject & TF_ATTN_INJECT) ? 1 : 0;
    // an edit's launches read the image `shift` branches in; its key norms too, unless the keys are the source's (injection)
    p.vt = w8 + vt_bytes(K, Spad, H, Dh, shift);
    p.knorm2 = reinterpret_cast<const float*>(w8 + vt_all) + (p.inject ? 0 : (size_t)shift * H * K * (Spad / 64));
    p.out = out;
    p.K = K;
    p.Kq = Kq;
    p.q_frame0 = q_frame0;
    p.S = S;
    p.H = H;
    p.Spad = Spad;
    p.nQT = (S + 127) / 128;
    p.part = inject & (TF_ATTN_BANK_ONLY | TF_ATTN_SOURCE_ONLY);
    p.fold = (inject & TF_ATTN_FOLD_SCALE) ? 1 : 0;
    p.out_f32 = (inject & TF_ATTN_OUT_F32) ? 1 : 0;
    p.nseg = split_plan(K_plan, Kq, S, H, Dh, p.inject != 0, p.part, !(inject & TF_ATTN_NO_SPLIT));
    p.Kb = Kb;
    if (sg) {   // a keyframe segment: its window of the whole bank's image and norm table
        p.vt = w8 + (size_t)sg->f0 * Spad * 2;
        p.knorm2 = reinterpret_cast<const float*>(w8 + vt_all) + (size_t)sg->f0 * (Spad / 64);
    }
    p.pslots = p.nseg > 1 ? p.nseg : 0;
    p.bit_stable = (inject & TF_ATTN_NO_SPLIT) ? 1 : 0;
    p.mix = (inject & TF_ATTN_HINT_MIX) ? 1 : 0;
    p.partials = reinterpret_cast<float*>(w8 + vt_all + kn_all);
    p.ld = ld;
    p.ld_q = ld_q;
    p.q_bs = strides[0];
    p.q_fs = strides[1];
    p.k_bs = strides[2];
    p.k_fs = strides[3];
    p.v_bs = strides[4];
    p.v_fs = strides[5];
    p.o_bs = strides[6];
    p.o_fs = strides[7];
    p.c = (float)((double)scale * 1.4426950408889634);
    p.gap = 2;
    if (ed) p.no_pack = ed->no_pack, p.mv4 = ed->mv4, p.force_dual = ed->force_dual, p.gap = ed->gap;
    if (sg) p.no_pack = 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (wn) {   // the same launches with the window table behind the parameter block
        // the split form's partial results: the workspace holds the worst case of the K-frame bank and the split is planned for
        // the longest window, a shorter bank -- checked here rather than assumed (no bank of up to 64 keyframes and no window
        // length is refused at the shapes swept in tests/test_windows_plan_cpu.py)
        TF_ARG((size_t)2 * Kq * H * S * p.pslots * (Dh + 8) <= attn_part_elems(K, S, H, Dh), TF_ERR_WORKSPACE,
               "tf_ext_attn_fwd_windows: %d partial-result slots do not fit the workspace of a %d-frame bank", p.pslots, K);
        AttnParamsWin pw{};
        static_cast<AttnParams&>(pw) = p;
        for (int i = 0; i < Kq; ++i) pw.win[i] = wn->win[i];
        return dtype == TF_BF16 ? dispatch_dh<BF16>(Dh, pw, v, st) : dispatch_dh<F16>(Dh, pw, v, st);
    }
    if (fs) {   // the same launches with the member masks behind the parameter block; the same check of the partial results
        TF_ARG((size_t)2 * Kq * H * S * p.pslots * (Dh + 8) <= attn_part_elems(K, S, H, Dh), TF_ERR_WORKSPACE,
               "tf_ext_attn_fwd_frame_sets: %d partial-result slots do not fit the workspace of a %d-frame bank", p.pslots, K);
        AttnParamsSet ps{};
        static_cast<AttnParams&>(ps) = p;
        for (int i = 0; i < Kq; ++i) ps.set[i] = fs->set[i];
        return dtype == TF_BF16 ? dispatch_dh<BF16>(Dh, ps, v, st) : dispatch_dh<F16>(Dh, ps, v, st);
    }
    return dtype == TF_BF16 ? dispatch_dh<BF16>(Dh, p, v, st) : dispatch_dh<F16>(Dh, p, v, st);
}

}  // namespace

extern "C" int tf_ext_attn_fwd_strided(const void* q, const void* k, const void* v, void* out, int K, int Kq,
                                       int q_frame0, int S, int H, int Dh, int64_t ld, const int64_t* strides,
                                       float scale, int inject, int dtype, void* ws, size_t ws_bytes, void* stream) {
    return attn_fwd_core(q, k, v, out, K, Kq, q_frame0, S, H, Dh, ld, strides, scale, inject, dtype, ws, ws_bytes, stream,
                         nullptr);
}

// ---------------------------------------------------------------------------------------------
// Multi-edit batches (include/tokenflow_hip.h): B = 1 + 2E branches [source | uncond_1 | cond_1 | ... ].  Composition of the
// single-edit parts: ONE V^T pre-pass over every branch a streaming launch reads, the source branch through the launches of a
// TF_ATTN_SOURCE_ONLY call, every edit's bank branches through those of a TF_ATTN_BANK_ONLY call on that edit's slabs -- the
// same kernels on the same values, so bit for bit the `part=` calls' results.  Under injection at Dh = 40 PAIRS of edits may
// take the four-bank shared-softmax launch instead (MODE_MV4; TF_ATTN_MULTI_V / TF_ATTN_NO_MULTI_V), at Dh = 64 behind
// TF_ATTN_MULTI_V64.
extern "C" size_t tf_ext_attn_edits_workspace_bytes(int K, int S, int H, int Dh, int n_edits, int dtype) {
    if (n_edits < 1 || n_edits > TF_MAX_EDITS) return 0;
    return attn_ws_bytes(K, S, H, Dh, dtype, 1 + 2 * n_edits);
}

// Default of the four-bank form where neither hint is given: only the shape classes in which it measured faster than the
// DUAL composition by more than the run-to-run spread (profiles/r08_attn_edits_ab.txt): every keyframe's queries (Kq = K),
// 8 heads, banks of 4 to 8 keyframes, frames of 1024 to 4096 tokens (-6 % / -17 % at E = 2, -3.5 % / -13 % at E = 3).
// Everything else -- query-frame subsets, other head counts, shorter or longer frames, larger banks -- was not measured and
// stays behind TF_ATTN_MULTI_V.
static bool mv4_default(int K, int Kq, int S, int H) {
    return Kq == K && H == 8 && K >= 4 && K <= 8 && S >= 1024 && S <= 4096;
}

// The same for the four-bank form at Dh = 64 (one<64,1,8,MV4,..>; profiles/r13_attn_edits_d64_ab.txt): ahead of the DUAL
// composition by far more than the run-to-run spread at the level-0 and level-1 shapes of BASELINE configs 4 and 5, for E = 2
// and E = 3 -- (K, S, H) = (10, 9216, 5): 28.9 against 36.7 ms, (25, 4096, 5): 31.5 / 42.4, (10, 2304, 10): 3.79 / 4.83,
// (25, 1024, 10): 4.18 / 5.42 at E = 2.  The rule is the box those four span: every keyframe's queries, 5 or 10 heads, banks
// of 10 to 25 keyframes, whole 64-key tiles, frames of 1024 to 9216 tokens.  Everything else -- smaller banks, other head
// counts, ragged or shorter frames, query-frame subsets -- was not measured and stays behind TF_ATTN_MULTI_V64.
static bool mv4_d64_default(int K, int Kq, int S, int H) {
    return Kq == K && (H == 5 || H == 10) && K >= 10 && K <= 25 && S % 64 == 0 && S >= 1024 && S <= 9216;
}

// The four-bank form in a WINDOWED multi-edit call (tf_ext_attn_fwd_windows_edits; K_max = the longest window).  The two rules
// above were measured on whole banks and say nothing about windows: this one comes from the three-arm A/B of
// profiles/r19_window_edits_ab.txt alone (E windowed single-edit calls / the DUAL composition / the four-bank form forced; radius
// 2 at the level-0 shapes of BASELINE configs 2, 4 and 5, E = 2 and 3), and holds only the shape classes in which the forced
// form is ahead of the DUAL composition by more than the run-to-run spread of both arms.  It is in all three, at E = 2 / E = 3
// (medians, spreads of 0.3 to 0.9 % per arm):
//   Dh = 64, (K, S, H) = (25, 4096, 5):  6.87 against  8.74 ms (-21 %) / 10.77 against 12.77 ms (-16 %)
//   Dh = 64, (K, S, H) = (10, 9216, 5): 13.33 against 16.79 ms (-21 %) / 21.21 against 24.56 ms (-14 %)
//   Dh = 40, (K, S, H) = (8, 4096, 8):   2.35 against  2.56 ms (-8 %)  /  3.49 against  3.67 ms (-5 %)
// The rule is what those cells span and no more: every keyframe's queries, a longest window of 5 frames (radius 2); at Dh = 64
// the box of the two shapes (5 heads, banks of 10 to 25 keyframes, whole 64-key tiles, frames of 4096 to 9216 tokens), at
// Dh = 40 the one shape.  Other radii, head counts, frame sizes, query-frame subsets and irregular tables with longer windows
// were not measured and stay behind TF_ATTN_MULTI_V / TF_ATTN_MULTI_V64.
static bool mv4_win_default(int K, int K_max, int Kq, int S, int H, int Dh) {
    if (Kq != K || K_max != 5) return false;
    if (Dh == 64) return H == 5 && K >= 10 && K <= 25 && S % 64 == 0 && S >= 4096 && S <= 9216;
    return Dh == 40 && H == 8 && K == 8 && S == 4096;
}

// The four-bank form in a FRAME-SET multi-edit call (tf_ext_attn_fwd_frame_sets_edits; K_max = the largest set).  The three rules
// above speak of whole banks or of radius-2 windows and say nothing about sets: this one is written from the three-arm A/B of
// profiles/r21_frame_sets_edits_ab.txt alone and covers only the shape classes in which the forced form is ahead of the DUAL
// composition by more than the run-to-run spread of both arms (E single-edit frame-set calls of the parent build / the DUAL
// composition / the four-bank form forced; radius 2 with anchor keyframe 0 -- a largest set of 6 frames -- at the level-0 shapes
// of BASELINE configs 2, 4 and 5, E = 2 and 3).  It is in all three, at E = 2 / E = 3 (medians, spreads of 0.1 to 1.5 % per arm):
//   Dh = 64, (K, S, H) = (25, 4096, 5):  7.96 against 10.40 ms (-23 %) / 12.65 against 15.21 ms (-17 %)
//   Dh = 64, (K, S, H) = (10, 9216, 5): 15.21 against 19.80 ms (-23 %) / 24.72 against 29.33 ms (-16 %)
//   Dh = 40, (K, S, H) = (8, 4096, 8):   2.72 against  2.94 ms (-8 %)  /  4.08 against  4.28 ms (-5 %)
// The rule is what those cells span and no more: every keyframe's queries, a largest set of 6 frames; at Dh = 64 the box of the
// two shapes (5 heads, banks of 10 to 25 keyframes, whole 64-key tiles, frames of 4096 to 9216 tokens), at Dh = 40 the one shape.
// Other radii and anchor counts, head counts, frame sizes and query-frame subsets were not measured and stay behind
// TF_ATTN_MULTI_V / TF_ATTN_MULTI_V64.
static bool mv4_set_default(int K, int K_max, int Kq, int S, int H, int Dh) {
    if (Kq != K || K_max != 6) return false;
    if (Dh == 64) return H == 5 && K >= 10 && K <= 25 && S % 64 == 0 && S >= 4096 && S <= 9216;
    return Dh == 40 && H == 8 && K == 8 && S == 4096;
}

// The masked composition: bit e of inject_mask = edit e injects (its uncond and cond branches use the source's q and k).
// tf_ext_attn_fwd_edits is the two uniform masks of it.
static int attn_fwd_edits_masked(const char* name, const void* q, const void* k, const void* v, void* out, int K, int Kq,
                                 int q_frame0, int S, int H, int Dh, int64_t ld, const int64_t* strides, float scale, int flags,
                                 int dtype, int n_edits, unsigned inject_mask, void* ws, size_t ws_bytes, void* stream,
                                 bool part_call = false, int qk_compact = 0, const WinPart* wn = nullptr,
                                 const SetPart* fs = nullptr) {
    TF_ARG(n_edits >= 1 && n_edits <= TF_MAX_EDITS, TF_ERR_SHAPE, "%s: n_edits=%d (1 .. %d)", name, n_edits, TF_MAX_EDITS);
    TF_ARG(q && k && v && out && ws && strides, TF_ERR_NULL, "%s: null pointer", name);
    TF_ARG(dtype == TF_BF16 || dtype == TF_F16, TF_ERR_DTYPE, "%s: dtype %d (bf16/f16 only)", name, dtype);
    // tf_ext_attn_fwd_edits_part (part_call): the parts of this composition; one-pass fused parts share ONE launch there
    const int part = flags & (TF_ATTN_BANK_ONLY | TF_ATTN_SOURCE_ONLY);
    if (part_call) {
        TF_ARG(part != (TF_ATTN_BANK_ONLY | TF_ATTN_SOURCE_ONLY), TF_ERR_SHAPE,
               "%s: TF_ATTN_BANK_ONLY and TF_ATTN_SOURCE_ONLY exclude each other", name);
        TF_ARG(qk_compact == 0 || qk_compact == 1, TF_ERR_SHAPE, "%s: qk_compact=%d (0 or 1)", name, qk_compact);
    } else {
        TF_ARG(!part, TF_ERR_SHAPE, "%s: TF_ATTN_BANK_ONLY / TF_ATTN_SOURCE_ONLY have no multi-edit form", name);
    }
    const bool do_bank = part != TF_ATTN_SOURCE_ONLY, do_src = part != TF_ATTN_BANK_ONLY;
    TF_ARG((flags & (TF_ATTN_MULTI_V | TF_ATTN_NO_MULTI_V)) != (TF_ATTN_MULTI_V | TF_ATTN_NO_MULTI_V), TF_ERR_SHAPE,
           "%s: TF_ATTN_MULTI_V and TF_ATTN_NO_MULTI_V exclude each other", name);
    TF_ARG((flags & (TF_ATTN_MULTI_V64 | TF_ATTN_NO_MULTI_V)) != (TF_ATTN_MULTI_V64 | TF_ATTN_NO_MULTI_V), TF_ERR_SHAPE,
           "%s: TF_ATTN_MULTI_V64 and TF_ATTN_NO_MULTI_V exclude each other", name);
    TF_ARG(!(flags & TF_ATTN_INJECT), TF_ERR_SHAPE, "%s: TF_ATTN_INJECT beside a mask (the mask is the injection state)", name);
    const unsigned all = (1u << n_edits) - 1u;
    TF_ARG(!(inject_mask & ~all), TF_ERR_SHAPE, "%s: inject_mask=0x%x has bits at or above n_edits=%d", name, inject_mask,
           n_edits);
    const int base = flags & ~(TF_ATTN_MULTI_V | TF_ATTN_MULTI_V64 | TF_ATTN_NO_MULTI_V | TF_ATTN_BANK_ONLY | TF_ATTN_SOURCE_ONLY);
    if (n_edits == 1)   // today's layout: today's call (the hints of the four-bank form have nothing to select); the compact
                        // q / k of one edit is the dense one as far as its launches read it
        return attn_fwd_core(q, k, v, out, K, Kq, q_frame0, S, H, Dh, ld, strides, scale,
                             base | part | (inject_mask ? TF_ATTN_INJECT : 0), dtype, ws, ws_bytes, stream, nullptr, nullptr, wn, fs);
    const int B = 1 + 2 * n_edits;
    int inj_e[TF_MAX_EDITS], non_e[TF_MAX_EDITS], n_inj = 0, n_non = 0;   // the injecting / the other edits, ascending
    int qk_sh[TF_MAX_EDITS];   // q / k branch slots in front of edit e's uncond slot, minus 1 (an injecting edit reads slot 0)
    for (int e = 0; e < n_edits; ++e) {
        qk_sh[e] = qk_compact ? 2 * n_non : 2 * e;
        ((inject_mask >> e) & 1u) ? inj_e[n_inj++] = e : non_e[n_non++] = e;
    }
    const int64_t osz = (flags & TF_ATTN_OUT_F32) ? 4 : 2;
    auto at = [](const void* ptr, int64_t elems, int64_t esz) {
        return static_cast<const void*>(static_cast<const unsigned char*>(ptr) + elems * esz);
    };
    // the four-bank form: Dh = 40 or 64 (each behind its own hint and its own measured default), fp32 score scaling, at least
    // one pair of INJECTING edits
    const bool mv_ok = n_inj >= 2 && (Dh == 40 || Dh == 64) && !(flags & TF_ATTN_FOLD_SCALE);
    // (the two measured defaults speak of whole banks: a windowed and a frame-set call have a rule of their own each)
    const bool mv_dflt = wn ? mv4_win_default(K, wn->K_max, Kq, S, H, Dh)
                       : fs ? mv4_set_default(K, fs->K_max, Kq, S, H, Dh)
                            : (Dh == 40 ? mv4_default(K, Kq, S, H) : mv4_d64_default(K, Kq, S, H));
    const bool mv_on = (flags & (Dh == 40 ? TF_ATTN_MULTI_V : TF_ATTN_MULTI_V64)) || mv_dflt;
    const bool mv = mv_ok && !(flags & TF_ATTN_NO_MULTI_V) && mv_on;
    // the pair launches and the odd edit beside them are one-pass streaming launches
    const int inj_flags = base | TF_ATTN_INJECT | TF_ATTN_BANK_ONLY | (mv ? TF_ATTN_NO_SPLIT | TF_ATTN_NO_FUSED : 0);
    const int non_flags = base | TF_ATTN_BANK_ONLY;
    // the source-only call sees TF_ATTN_INJECT iff every edit injects (its result does not depend on the flag: the source
    // branch reads its own q and k either way; its split decision may)
    const int src_flags = base | TF_ATTN_SOURCE_ONLY | (n_non == 0 ? TF_ATTN_INJECT : 0);
    auto call = [&](int e, int fl, const EditsPart& ed) {   // the part `fl` of edit e (e = 0 for the source branch)
        const int sh = 2 * e;
        const bool inj = (fl & TF_ATTN_INJECT) != 0;
        const int qsh = (fl & TF_ATTN_SOURCE_ONLY) ? 0 : qk_sh[e];
        // a sliding-window bank (tf_ext_attn_fwd_windows_edits) or a frame-set bank (tf_ext_attn_fwd_frame_sets_edits): every bank
        // part reads the table; the source part is the plain source-only call (a source problem reads its own frame whatever
        // the table)
        return attn_fwd_core(inj ? q : at(q, qsh * strides[0], 2), inj ? k : at(k, qsh * strides[2], 2), at(v, sh * strides[4], 2),
                             const_cast<void*>(at(out, sh * strides[6], osz)), K, Kq, q_frame0, S, H, Dh, ld, strides, scale, fl,
                             dtype, ws, ws_bytes, stream, &ed, nullptr, (fl & TF_ATTN_SOURCE_ONLY) ? nullptr : wn,
                             (fl & TF_ATTN_SOURCE_ONLY) ? nullptr : fs);
    };
    // which parts stream (and read the V^T image): the decision of the part's own call
    const EditsPart probe = EditsPart::probe_of(B);
    const int src_fused = call(0, src_flags, probe);   // (a bank part decides its pre-pass as the whole call does)
    if (src_fused < 0) return src_fused;
    const int inj_fused = n_inj && do_bank ? call(0, inj_flags, probe) : 1;
    if (inj_fused < 0) return inj_fused;
    const int non_fused = n_non && do_bank ? call(0, non_flags, probe) : 1;
    if (non_fused < 0) return non_fused;
    if (part_call && (src_fused || !do_src) && inj_fused && non_fused) {
        // every part this call computes takes the fused small-problem kernel: ONE launch over all of them, a set per edit's
        // bank branches (the order of the streaming composition) and the source set; the injection state is the set's
        TfAttnSet sets[1 + TF_MAX_EDITS] = {};
        int n_sets = 0;
        auto add = [&](int e, int b0, int nb, bool inj) {
            TfAttnSet& a = sets[n_sets++];
            const int sh = b0 ? 2 * e : 0, qsh = b0 && !inj ? qk_sh[e] : 0;
            a.q = at(q, qsh * strides[0], 2), a.k = at(k, qsh * strides[2], 2), a.v = at(v, sh * strides[4], 2);
            a.out = const_cast<void*>(at(out, sh * strides[6], osz));
            a.q_bs = strides[0], a.q_fs = strides[1], a.ld_q = strides[8];
            a.k_bs = strides[2], a.k_fs = strides[3], a.v_bs = strides[4], a.v_fs = strides[5], a.ld = ld;
            a.o_bs = strides[6], a.o_fs = strides[7];
            a.H = H, a.Kq = Kq, a.q_frame0 = q_frame0, a.Kb = K, a.b0 = b0, a.nb = nb, a.inject = inj ? 1 : 0;
        };
        if (do_bank) {
            for (int i = 0; i < n_inj; ++i) add(inj_e[i], 1, 2, true);
            for (int i = 0; i < n_non; ++i) add(non_e[i], 1, 2, false);
        }
        if (do_src) add(0, 0, 1, false);
        const int fl = base;   // no launch-wide TF_ATTN_INJECT: every set carries its own
        // a windowed / frame-set part (tf_ext_attn_fwd_windows_edits_part, tf_ext_attn_fwd_frame_sets_edits_part): planned for the
        // longest window / largest set, as the one-set windowed launch is, and launched under the ONE table all edits share
        const int K_plan = wn ? wn->K_max : fs ? fs->K_max : K;
        for (int i = 0; i < n_sets; ++i) sets[i].Kb = K_plan;
        const TfFusedPlan plan = tf_attn_fused_plan(sets, n_sets, S, Dh, dtype, fl);
        for (int i = 0; i < n_sets; ++i) sets[i].Kb = K;
        // (the default mode decides per grid: where the joint grid leaves the fused kernel's range, the parts run as below)
        if (plan.use) {
            TF_ARG(Kq > 0 && q_frame0 >= 0 && q_frame0 + Kq <= K && K > 0 && S > 0 && H > 0, TF_ERR_SHAPE,
                   "%s: query frames [%d, %d) outside the %d-frame bank", name, q_frame0, q_frame0 + Kq, K);
            return tf_attn_fused_launch(sets, n_sets, S, Dh, scale, fl, dtype, plan, reinterpret_cast<hipStream_t>(stream),
                                        do_bank && wn ? wn->win : nullptr, do_bank && fs ? fs->set : nullptr);
        }
    }
    // ONE pre-pass over the span of the streaming branches; key norms of every packed branch whose OWN keys a launch reads
    // (the source, the edits that do not inject); where an injecting edit streams beside a fused source part, the workgroups
    // of the first injecting branch compute the source's norms, as in the single-edit call under injection
    int b_lo = B, b_hi = 0;
    unsigned own = 0;
    auto span = [&](int lo, int hi) { b_lo = lo < b_lo ? lo : b_lo, b_hi = hi > b_hi ? hi : b_hi; };
    if (!src_fused && do_src) span(0, 1), own |= 1u;
    if (!inj_fused)
        for (int i = 0; i < n_inj; ++i) span(1 + 2 * inj_e[i], 3 + 2 * inj_e[i]);
    if (!non_fused)
        for (int i = 0; i < n_non; ++i) span(1 + 2 * non_e[i], 3 + 2 * non_e[i]), own |= 3u << (1 + 2 * non_e[i]);
    if (b_lo < b_hi) {
        const int Spad = ((S + 127) / 128) * 128;
        AttnParams p{};
        p.k = k, p.vt = ws;
        p.knorm2 = reinterpret_cast<const float*>(static_cast<unsigned char*>(ws) + ((vt_bytes(K, Spad, H, Dh, B) + 255) & ~(size_t)255));
        p.K = p.Kb = K, p.S = S, p.H = H, p.Spad = Spad, p.nseg = 1;
        p.ld = ld, p.k_bs = strides[2], p.k_fs = strides[3], p.v_bs = strides[4], p.v_fs = strides[5];
        const int b_src = (!inj_fused && (src_fused || !do_src)) ? 1 + 2 * inj_e[0] : -1;
        const unsigned kc_mask = qk_compact ? inject_mask : 0u;
        hipStream_t st = reinterpret_cast<hipStream_t>(stream);
        const int rc = dtype == TF_BF16 ? launch_vt_pack<BF16>(p, v, Dh, b_lo, b_hi, own, b_src, st, kc_mask)
                                        : launch_vt_pack<F16>(p, v, Dh, b_lo, b_hi, own, b_src, st, kc_mask);
        if (rc) return rc;
    }
    // bank branches first (the long problems), then the source branch, as the single-edit call orders them: the injecting
    // edits (pairs in the four-bank form, an odd last one in the DUAL launch beside them), then the others
    int i = 0;
    if (!do_bank) return call(0, src_flags, EditsPart::source(B));
    if (mv)
        for (; i + 2 <= n_inj; i += 2)
            if (const int rc = call(inj_e[i], inj_flags, EditsPart::pair_mv4(B, inj_e[i], inj_e[i + 1]))) return rc;
    for (; i < n_inj; ++i)
        if (const int rc = call(inj_e[i], inj_flags, mv ? EditsPart::bank_dual(B, inj_e[i]) : EditsPart::bank(B, inj_e[i])))
            return rc;
    for (i = 0; i < n_non; ++i)
        if (const int rc = call(non_e[i], non_flags, EditsPart::bank(B, non_e[i]))) return rc;
    return do_src ? call(0, src_flags, EditsPart::source(B)) : 0;
}

extern "C" int tf_ext_attn_fwd_edits(const void* q, const void* k, const void* v, void* out, int K, int Kq, int q_frame0,
                                     int S, int H, int Dh, int64_t ld, const int64_t* strides, float scale, int flags,
                                     int dtype, int n_edits, void* ws, size_t ws_bytes, void* stream) {
    const unsigned all = (n_edits >= 1 && n_edits <= TF_MAX_EDITS) ? (1u << n_edits) - 1u : 0u;
    return attn_fwd_edits_masked("tf_ext_attn_fwd_edits", q, k, v, out, K, Kq, q_frame0, S, H, Dh, ld, strides, scale,
                                 flags & ~TF_ATTN_INJECT, dtype, n_edits, (flags & TF_ATTN_INJECT) ? all : 0u, ws, ws_bytes,
                                 stream);
}

extern "C" int tf_ext_attn_fwd_edits_masked(const void* q, const void* k, const void* v, void* out, int K, int Kq,
                                            int q_frame0, int S, int H, int Dh, int64_t ld, const int64_t* strides,
                                            float scale, int flags, int dtype, int n_edits, unsigned inject_mask, void* ws,
                                            size_t ws_bytes, void* stream) {
    return attn_fwd_edits_masked("tf_ext_attn_fwd_edits_masked", q, k, v, out, K, Kq, q_frame0, S, H, Dh, ld, strides, scale,
                                 flags, dtype, n_edits, inject_mask, ws, ws_bytes, stream);
}

// The parts of the masked composition (include/tokenflow_hip.h): a frame-sharded rank computes the bank branches of every
// edit on the buffer its exchange delivered and the source branch on its own tensors.
extern "C" int tf_ext_attn_fwd_edits_part(const void* q, const void* k, const void* v, void* out, int K, int Kq, int q_frame0,
                                          int S, int H, int Dh, int64_t ld, const int64_t* strides, float scale, int flags,
                                          int dtype, int n_edits, unsigned inject_mask, int qk_compact, void* ws,
                                          size_t ws_bytes, void* stream) {
    return attn_fwd_edits_masked("tf_ext_attn_fwd_edits_part", q, k, v, out, K, Kq, q_frame0, S, H, Dh, ld, strides, scale,
                                 flags, dtype, n_edits, inject_mask, ws, ws_bytes, stream, true, qk_compact);
}

// Launch plan of tf_ext_attn_fwd_edits_part for dense tensors (q / k dense or compact: the plan does not depend on it).
extern "C" int tf_ext_attn_edits_part_plan(int K, int Kq, int S, int H, int Dh, int n_edits, unsigned inject_mask,
                                           int qk_compact, int flags, int dtype, char* buf, size_t len) {
    TF_ARG(K > 0 && S > 0 && H > 0 && Kq > 0 && Kq <= K, TF_ERR_SHAPE, "tf_ext_attn_edits_part_plan: K=%d Kq=%d S=%d H=%d", K,
           Kq, S, H);
    void* const ph = reinterpret_cast<void*>((uintptr_t)1 << 12);
    const int64_t ld = (int64_t)H * Dh, fs = (int64_t)S * ld;
    const int64_t strides[9] = {Kq * fs, fs, K * fs, fs, K * fs, fs, Kq * fs, fs, ld};
    TfPlanRec rec{buf, len, 0, 0};
    if (buf && len) buf[0] = 0;
    tf_plan_rec = &rec;
    const int rc = tf_ext_attn_fwd_edits_part(ph, ph, ph, ph, K, Kq, 0, S, H, Dh, ld, strides, 1.0f, flags, dtype, n_edits,
                                              inject_mask, qk_compact, ph, (size_t)-1, nullptr);
    tf_plan_rec = nullptr;
    if (rc) return rc;
    TF_ARG(rec.used < len, TF_ERR_WORKSPACE, "tf_ext_attn_edits_part_plan: the plan needs %zu bytes", rec.used + 1);
    return rec.n;
}

// Launch plan of tf_ext_attn_fwd_edits for dense tensors, recorded by the entry point itself as tf_ext_attn_plan does.
extern "C" int tf_ext_attn_edits_plan(int K, int Kq, int S, int H, int Dh, int n_edits, int flags, int dtype, char* buf,
                                      size_t len) {
    TF_ARG(K > 0 && S > 0 && H > 0 && Kq > 0 && Kq <= K, TF_ERR_SHAPE, "tf_ext_attn_edits_plan: K=%d Kq=%d S=%d H=%d", K, Kq,
           S, H);
    void* const ph = reinterpret_cast<void*>((uintptr_t)1 << 12);
    const int64_t ld = (int64_t)H * Dh, fs = (int64_t)S * ld;
    const int64_t strides[9] = {Kq * fs, fs, K * fs, fs, K * fs, fs, Kq * fs, fs, ld};
    TfPlanRec rec{buf, len, 0, 0};
    if (buf && len) buf[0] = 0;
    tf_plan_rec = &rec;
    const int rc = tf_ext_attn_fwd_edits(ph, ph, ph, ph, K, Kq, 0, S, H, Dh, ld, strides, 1.0f, flags, dtype, n_edits, ph,
                                         (size_t)-1, nullptr);
    tf_plan_rec = nullptr;
    if (rc) return rc;
    TF_ARG(rec.used < len, TF_ERR_WORKSPACE, "tf_ext_attn_edits_plan: the plan needs %zu bytes", rec.used + 1);
    return rec.n;
}

// The same for tf_ext_attn_fwd_edits_masked.
extern "C" int tf_ext_attn_edits_masked_plan(int K, int Kq, int S, int H, int Dh, int n_edits, unsigned inject_mask, int flags,
                                             int dtype, char* buf, size_t len) {
    TF_ARG(K > 0 && S > 0 && H > 0 && Kq > 0 && Kq <= K, TF_ERR_SHAPE, "tf_ext_attn_edits_masked_plan: K=%d Kq=%d S=%d H=%d", K,
           Kq, S, H);
    void* const ph = reinterpret_cast<void*>((uintptr_t)1 << 12);
    const int64_t ld = (int64_t)H * Dh, fs = (int64_t)S * ld;
    const int64_t strides[9] = {Kq * fs, fs, K * fs, fs, K * fs, fs, Kq * fs, fs, ld};
    TfPlanRec rec{buf, len, 0, 0};
    if (buf && len) buf[0] = 0;
    tf_plan_rec = &rec;
    const int rc = tf_ext_attn_fwd_edits_masked(ph, ph, ph, ph, K, Kq, 0, S, H, Dh, ld, strides, 1.0f, flags, dtype, n_edits,
                                                inject_mask, ph, (size_t)-1, nullptr);
    tf_plan_rec = nullptr;
    if (rc) return rc;
    TF_ARG(rec.used < len, TF_ERR_WORKSPACE, "tf_ext_attn_edits_masked_plan: the plan needs %zu bytes", rec.used + 1);
    return rec.n;
}

// ---------------------------------------------------------------------------------------------
// Runs form: attention over a bank that arrives in pieces (include/tokenflow_hip.h, "run + merge").
//
// Workspace of one run SET: V^T image of the whole bank | key norm bounds of the whole bank | slots filled per run (n_runs
// ints) | partial results [2 banks][Kq][H][S][n_runs * spr][Dh + 8] fp32.  Every run writes only the positions of its own
// frames in the first two, its own int in the third and its own spr slots in the last: the runs of one bank may execute
// concurrently.
namespace {

struct RunsLayout {
    int Spad, spr;   // spr = slots per run
    size_t knorm_off, hdr_off, part_off, part_edit, bytes;   // part_edit: floats of ONE edit's partial results
};

// Slots a run owns: the largest split any run of this bank can take (split_plan never grows when the frame count shrinks).
static int runs_slots_per_run(int K, int Kq, int S, int H, int Dh) {
    const int a = split_plan(K, Kq, S, H, Dh, false, 0, true), b = split_plan(K, Kq, S, H, Dh, true, 0, true);
    return a > b ? a : b;
}

// n_edits > 1 (tf_ext_attn_run_edits): the image and the norm table of all 1 + 2E branches, ONE header of n_runs ints (both
// injection states' slot counts in each, see attn_runs_merge_edits_kernel) and the partial results of every edit one behind the
// other, [2E][Kq][H][S][n_runs * spr][Dh + 8]: an edit's launches see the layout of a single-edit run set.
static RunsLayout runs_layout(int K, int Kq, int S, int H, int Dh, int n_runs, int n_edits = 1) {
    RunsLayout L;
    const int branches = 1 + 2 * n_edits;
    L.Spad = ((S + 127) / 128) * 128;
    L.spr = runs_slots_per_run(K, Kq, S, H, Dh);
    L.knorm_off = (vt_bytes(K, L.Spad, H, Dh, branches) + 255) & ~(size_t)255;
    L.hdr_off = L.knorm_off + (((size_t)branches * H * K * (L.Spad / 64) * sizeof(float) + 255) & ~(size_t)255);
    L.part_off = L.hdr_off + (((size_t)n_runs * sizeof(int) + 255) & ~(size_t)255);
    L.part_edit = (size_t)2 * Kq * H * S * n_runs * L.spr * (Dh + 8);
    L.bytes = L.part_off + (size_t)n_edits * L.part_edit * sizeof(float);
    return L;
}

static int runs_check_shape(const char* fn, int K, int Kq, int S, int H, int Dh, int n_runs, int dtype) {
    TF_ARG(dtype == TF_BF16 || dtype == TF_F16, TF_ERR_DTYPE, "%s: dtype %d (bf16/f16 only)", fn, dtype);
    TF_ARG(Dh == 40 || Dh == 64 || Dh == 80 || Dh == 160, TF_ERR_SHAPE, "%s: head dim %d not in {40,64,80,160}", fn, Dh);
    TF_ARG(K > 0 && S > 0 && H > 0 && Kq > 0 && Kq <= K, TF_ERR_SHAPE, "%s: K=%d Kq=%d S=%d H=%d", fn, K, Kq, S, H);
    TF_ARG(n_runs >= 1 && n_runs <= K, TF_ERR_SHAPE, "%s: %d runs over a bank of %d frames", fn, n_runs, K);
    return 0;
}

// flag bits a run call refuses: it always takes the streaming kernels, and the source branch alone has no bank to run over
constexpr int RUN_REFUSED = TF_ATTN_SOURCE_ONLY | TF_ATTN_FUSED | TF_ATTN_HINT_QW(7) | TF_ATTN_HINT_KW(7) | TF_ATTN_HINT_QB2 |
                            TF_ATTN_PRECISE_P | TF_ATTN_NO_PRECISE_P;

// One part of a multi-edit run call (tf_ext_attn_run_edits) as seen by the single-edit run call that computes it: the caller
// has moved the base pointers of q / k / v / out to the edit's slabs and packed the run's frames of every branch; the launches
// read the image (and, unless the edit injects, the norm table) `shift` branches in and leave the partial results in the
// edit's own region.
struct RunEditsPart {
    int n_edits;    // edits of the workspace layout
    int edit;       // whose partial region: shift = 2 * edit
    int src_only;   // the source branch of the query frames alone (edit = 0)
    int mv4_gap;    // > 0: ONE four-bank launch for `edit` and the injecting edit mv4_gap branches behind it (2 = the next edit)

    static RunEditsPart bank(int n_edits, int e) { return RunEditsPart{n_edits, e, 0, 0}; }
    static RunEditsPart pair_mv4(int n_edits, int e0, int e1) { return RunEditsPart{n_edits, e0, 0, 2 * (e1 - e0)}; }
    static RunEditsPart source(int n_edits) { return RunEditsPart{n_edits, 0, 1, 0}; }
};

// What a run call checks before anything touches the device.
static int attn_run_check(const char* fn, const void* q, const void* k, const void* v, const void* out, int K, int Kq,
                          int q_frame0, int run_f0, int run_n, int run, int n_runs, int S, int H, int Dh, int64_t ld,
                          const int64_t* strides, int flags, int dtype, const void* ws, size_t ws_bytes, int n_edits) {
    TF_ARG(q && k && v && out && ws && strides, TF_ERR_NULL, "%s: null pointer", fn);
    if (const int rc = runs_check_shape(fn, K, Kq, S, H, Dh, n_runs, dtype)) return rc;
    TF_ARG(ld >= (int64_t)H * Dh && ld % 8 == 0, TF_ERR_SHAPE, "%s: ld=%lld (a multiple of 8, >= H*Dh)", fn, (long long)ld);
    TF_ARG(q_frame0 >= 0 && q_frame0 + Kq <= K, TF_ERR_SHAPE, "%s: query frames [%d, %d) outside the %d-frame bank", fn,
           q_frame0, q_frame0 + Kq, K);
    TF_ARG(run >= 0 && run < n_runs, TF_ERR_SHAPE, "%s: run %d of %d", fn, run, n_runs);
    TF_ARG(run_n >= 1 && run_f0 >= 0 && run_f0 <= K - run_n, TF_ERR_SHAPE,
           "%s: run of frames [%d, %d) empty or outside the %d-frame bank", fn, run_f0, run_f0 + run_n, K);
    TF_ARG(!(flags & RUN_REFUSED), TF_ERR_SHAPE,
           "%s: flags 0x%x -- TF_ATTN_SOURCE_ONLY, TF_ATTN_FUSED and the fused kernel's hints have no run form", fn,
           flags & RUN_REFUSED);
    const bool bank_only = (flags & TF_ATTN_BANK_ONLY) != 0;
    TF_ARG(bank_only || (q_frame0 >= run_f0 && q_frame0 + Kq <= run_f0 + run_n), TF_ERR_SHAPE,
           "%s: the source branch needs the query frames [%d, %d) inside the run [%d, %d) "
           "(TF_ATTN_BANK_ONLY for the other runs)", fn, q_frame0, q_frame0 + Kq, run_f0, run_f0 + run_n);
    const int64_t ld_q = strides[8];
    TF_ARG(ld_q >= (int64_t)H * Dh && ld_q % 8 == 0, TF_ERR_SHAPE, "%s: q token stride %lld (a multiple of 8, >= H*Dh)", fn,
           (long long)ld_q);
    for (int i = 0; i < 8; ++i)
        TF_ARG(strides[i] % 8 == 0 &&
                   (i & 1 ? strides[i] >= (int64_t)(S - 1) * (i < 2 ? ld_q : i < 6 ? ld : (int64_t)H * Dh) : true),
               TF_ERR_SHAPE, "%s: stride %d = %lld (multiples of 8 elements; a frame holds S token rows)", fn, i,
               (long long)strides[i]);
    TF_ARG(tf_aligned16(q) && tf_aligned16(k) && tf_aligned16(v) && tf_aligned16(out) && tf_aligned16(ws), TF_ERR_ALIGN,
           "%s: tensors not 16-byte aligned", fn);
    const size_t need = runs_layout(K, Kq, S, H, Dh, n_runs, n_edits).bytes;
    TF_ARG(ws_bytes >= need, TF_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws_bytes, need);
    return 0;
}

int attn_run_core(const char* fn, const void* q, const void* k, const void* v, void* out, int K, int Kq, int q_frame0,
                  int run_f0, int run_n, int run, int n_runs, int S, int H, int Dh, int64_t ld, const int64_t* strides,
                  float scale, int flags, int dtype, void* ws, size_t ws_bytes, void* stream, const RunEditsPart* ed) {
    const int n_edits = ed ? ed->n_edits : 1;
    if (const int rc = attn_run_check(fn, q, k, v, out, K, Kq, q_frame0, run_f0, run_n, run, n_runs, S, H, Dh, ld, strides, flags,
                                      dtype, ws, ws_bytes, n_edits))
        return rc;
    const bool bank_only = (flags & TF_ATTN_BANK_ONLY) != 0;
    const int64_t ld_q = strides[8];
    const RunsLayout L = runs_layout(K, Kq, S, H, Dh, n_runs, n_edits);
    const int shift = ed ? 2 * ed->edit : 0;

    unsigned char* const w8 = static_cast<unsigned char*>(ws);
    const int ppf = L.Spad / 64;
    AttnParams p{};
    // the frame window is folded into K and the base pointers: the kernels see a bank of run_n frames that starts at run_f0
    // (frame f of the caller's k / v lives at base + f * frame stride; the V^T image and the norm table keep the whole
    // bank's row strides, p.Kb)
    p.q = q;
    p.k = static_cast<const unsigned char*>(k) + (int64_t)run_f0 * strides[3] * 2;
    const void* v_run = static_cast<const unsigned char*>(v) + (int64_t)run_f0 * strides[5] * 2;
    p.inject = (flags & TF_ATTN_INJECT) ? 1 : 0;
    // an edit's launches read the image `shift` branches in; its key norms too, unless the keys are the source's (injection)
    p.vt = w8 + vt_bytes(K, L.Spad, H, Dh, shift) + (size_t)run_f0 * L.Spad * 2;
    p.knorm2 = reinterpret_cast<const float*>(w8 + L.knorm_off) + (p.inject ? 0 : (size_t)shift * H * K * ppf) +
               (size_t)run_f0 * ppf;
    p.out = out;
    p.K = run_n;
    p.Kb = K;
    p.Kq = Kq;
    p.q_frame0 = bank_only ? 0 : q_frame0 - run_f0;
    p.S = S;
    p.H = H;
    p.Spad = L.Spad;
    p.nQT = (S + 127) / 128;
    p.part = (ed && ed->src_only) ? TF_ATTN_SOURCE_ONLY : bank_only ? TF_ATTN_BANK_ONLY : 0;
    p.fold = (flags & TF_ATTN_FOLD_SCALE) ? 1 : 0;
    p.out_f32 = (flags & TF_ATTN_OUT_F32) ? 1 : 0;
    const int ns = split_plan(run_n, Kq, S, H, Dh, p.inject != 0, p.part, !(flags & TF_ATTN_NO_SPLIT));
    p.nseg = ns < L.spr ? ns : L.spr;
    p.pslots = n_runs * L.spr;
    p.run = 1;
    p.run_hdr = reinterpret_cast<int*>(w8 + L.hdr_off) + run;
    p.bit_stable = 1;   // the kernel choice of a run is a function of its arguments: the mixed-shape form only on TF_ATTN_HINT_MIX
    p.mix = (flags & TF_ATTN_HINT_MIX) ? 1 : 0;
    p.partials = reinterpret_cast<float*>(w8 + L.part_off) + (ed ? (size_t)ed->edit * L.part_edit : 0) +
                 (size_t)run * L.spr * (Dh + 8);
    p.ld = ld;
    p.ld_q = ld_q;
    p.q_bs = strides[0];
    p.q_fs = strides[1];
    p.k_bs = strides[2];
    p.k_fs = strides[3];
    p.v_bs = strides[4];
    p.v_fs = strides[5];
    p.o_bs = strides[6];
    p.o_fs = strides[7];
    p.c = (float)((double)scale * 1.4426950408889634);
    p.gap = 2;
    // a pair of injecting edits in the four-bank form: banks 2 and 3 are the second edit's, in the image and in the partial
    // results alike (the edits' partial regions are one array of 2E branches, p.partials points into the first edit's)
    if (ed && ed->mv4_gap) p.mv4 = 1, p.gap = ed->mv4_gap;
    p.no_pack = ed ? 1 : 0;   // the composing call has packed the run's frames of every branch
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dtype == TF_BF16 ? dispatch_dh<BF16>(Dh, p, v_run, st) : dispatch_dh<F16>(Dh, p, v_run, st);
}

int attn_runs_merge_core(const char* fn, void* out, int K, int Kq, int S, int H, int Dh, int n_runs, int n_edits,
                         unsigned inject_mask, int64_t out_branch_stride, int64_t out_frame_stride, int flags, int dtype,
                         void* ws, size_t ws_bytes, void* stream) {
    TF_ARG(out && ws, TF_ERR_NULL, "%s: null pointer", fn);
    if (const int rc = runs_check_shape(fn, K, Kq, S, H, Dh, n_runs, dtype)) return rc;
    TF_ARG(out_branch_stride % 8 == 0 && out_frame_stride % 8 == 0 && out_frame_stride >= (int64_t)(S - 1) * H * Dh,
           TF_ERR_SHAPE, "%s: out strides %lld, %lld (multiples of 8 elements; a frame holds S token rows)", fn,
           (long long)out_branch_stride, (long long)out_frame_stride);
    TF_ARG(tf_aligned16(out) && tf_aligned16(ws), TF_ERR_ALIGN, "%s: tensors not 16-byte aligned", fn);
    const RunsLayout L = runs_layout(K, Kq, S, H, Dh, n_runs, n_edits);
    TF_ARG(ws_bytes >= L.bytes, TF_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws_bytes, L.bytes);
    if (n_edits == 1 ? tf_plan_note("merge[runs=%d]", n_runs) : tf_plan_note("merge[runs=%d,edits=%d]", n_runs, n_edits))
        return 0;
    unsigned char* const w8 = static_cast<unsigned char*>(ws);
    const int64_t total = (int64_t)2 * n_edits * Kq * H * S * (Dh / 4);
    const int64_t blocks = (total + 255) / 256;
    const dim3 grid((unsigned)(blocks < 8192 ? blocks : 8192));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const float* part = reinterpret_cast<const float*>(w8 + L.part_off);
    const int* hdr = reinterpret_cast<const int*>(w8 + L.hdr_off);
    const int f32 = (flags & TF_ATTN_OUT_F32) ? 1 : 0;
    if (n_edits > 1) {
        if (dtype == TF_BF16)
            hipLaunchKernelGGL(attn_runs_merge_edits_kernel<BF16>, grid, dim3(256), 0, st, part, hdr, out, Kq, S, H, Dh, n_runs,
                               L.spr, 2 * n_edits, inject_mask, f32, out_branch_stride, out_frame_stride);
        else
            hipLaunchKernelGGL(attn_runs_merge_edits_kernel<F16>, grid, dim3(256), 0, st, part, hdr, out, Kq, S, H, Dh, n_runs,
                               L.spr, 2 * n_edits, inject_mask, f32, out_branch_stride, out_frame_stride);
    } else if (dtype == TF_BF16)
        hipLaunchKernelGGL(attn_runs_merge_kernel<BF16>, grid, dim3(256), 0, st, part, hdr, out, Kq, S, H, Dh, n_runs, L.spr, f32,
                           out_branch_stride, out_frame_stride);
    else
        hipLaunchKernelGGL(attn_runs_merge_kernel<F16>, grid, dim3(256), 0, st, part, hdr, out, Kq, S, H, Dh, n_runs, L.spr, f32,
                           out_branch_stride, out_frame_stride);
    TF_LAUNCH_CHECK(fn);
    return 0;
}

// What the multi-edit run and merge calls check of their own arguments.
static int run_edits_check(const char* fn, int n_edits, unsigned inject_mask, int flags) {
    TF_ARG(n_edits >= 1 && n_edits <= TF_MAX_EDITS, TF_ERR_SHAPE, "%s: n_edits=%d (1 .. %d)", fn, n_edits, TF_MAX_EDITS);
    TF_ARG(!(flags & TF_ATTN_INJECT), TF_ERR_SHAPE, "%s: TF_ATTN_INJECT beside a mask (the mask is the injection state)", fn);
    TF_ARG(!(inject_mask & ~((1u << n_edits) - 1u)), TF_ERR_SHAPE, "%s: inject_mask=0x%x has bits at or above n_edits=%d", fn,
           inject_mask, n_edits);
    TF_ARG(!(flags & (TF_ATTN_MULTI_V | TF_ATTN_MULTI_V64)), TF_ERR_SHAPE,
           "%s: TF_ATTN_MULTI_V / TF_ATTN_MULTI_V64 -- the one-call hints select nothing in a run, whose four-bank form is opted into "
           "with TF_ATTN_RUN_MULTI_V",
           fn);
    return 0;
}

}  // namespace

extern "C" size_t tf_ext_attn_runs_workspace_bytes(int K, int Kq, int S, int H, int Dh, int n_runs, int dtype) {
    if (K <= 0 || Kq <= 0 || Kq > K || S <= 0 || H <= 0 || n_runs <= 0 || n_runs > K || dtype == TF_F32) return 0;
    if (!(Dh == 40 || Dh == 64 || Dh == 80 || Dh == 160)) return 0;
    return runs_layout(K, Kq, S, H, Dh, n_runs).bytes;
}

extern "C" int tf_ext_attn_run(const void* q, const void* k, const void* v, void* out, int K, int Kq, int q_frame0,
                               int run_f0, int run_n, int run, int n_runs, int S, int H, int Dh, int64_t ld,
                               const int64_t* strides, float scale, int flags, int dtype, void* ws, size_t ws_bytes,
                               void* stream) {
    return attn_run_core("tf_ext_attn_run", q, k, v, out, K, Kq, q_frame0, run_f0, run_n, run, n_runs, S, H, Dh, ld, strides,
                         scale, flags, dtype, ws, ws_bytes, stream, nullptr);
}

extern "C" int tf_ext_attn_runs_merge(void* out, int K, int Kq, int S, int H, int Dh, int n_runs, int64_t out_branch_stride,
                                      int64_t out_frame_stride, int flags, int dtype, void* ws, size_t ws_bytes,
                                      void* stream) {
    return attn_runs_merge_core("tf_ext_attn_runs_merge", out, K, Kq, S, H, Dh, n_runs, 1, 0u, out_branch_stride,
                                out_frame_stride, flags, dtype, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------------------------------------
// Runs form of a multi-edit batch (include/tokenflow_hip.h): attn_fwd_edits_masked applied to a run.  ONE V^T pre-pass per run
// call over the run's frames of every branch the call reads, at their positions in the image of the whole bank (key norms of
// the source and of the edits that do not inject; in a bank-only call under injection the first injecting branch computes
// the source's), then every edit's bank branches through the launches of its own tf_ext_attn_run call -- base pointers 2e
// branches in: q / k unless injected, v, out, the image, the norm table, the edit's partial region -- then the source branch.
// No fused kernel: it has no partial epilogue.  With TF_ATTN_RUN_MULTI_V (Dh = 40, 64, fp32 score scaling) the injecting edits
// are paired ascending and each pair is ONE four-bank run launch (MODE_MV4) over the source's q / k: it splits into the slots
// the pre-pass header records for the injecting state and leaves each edit's partial rows in that edit's region, so the
// header, the layout and the merge are those of the DUAL composition.
extern "C" size_t tf_ext_attn_runs_edits_workspace_bytes(int K, int Kq, int S, int H, int Dh, int n_runs, int n_edits,
                                                         int dtype) {
    if (n_edits < 1 || n_edits > TF_MAX_EDITS) return 0;
    if (K <= 0 || Kq <= 0 || Kq > K || S <= 0 || H <= 0 || n_runs <= 0 || n_runs > K || dtype == TF_F32) return 0;
    if (!(Dh == 40 || Dh == 64 || Dh == 80 || Dh == 160)) return 0;
    return runs_layout(K, Kq, S, H, Dh, n_runs, n_edits).bytes;
}

extern "C" int tf_ext_attn_run_edits(const void* q, const void* k, const void* v, void* out, int K, int Kq, int q_frame0,
                                     int run_f0, int run_n, int run, int n_runs, int S, int H, int Dh, int64_t ld,
                                     const int64_t* strides, float scale, int flags, int dtype, int n_edits,
                                     unsigned inject_mask, int compact, void* ws, size_t ws_bytes, void* stream) {
    const char* const fn = "tf_ext_attn_run_edits";
    if (const int rc = run_edits_check(fn, n_edits, inject_mask, flags)) return rc;
    TF_ARG(compact >= 0 && compact <= 3, TF_ERR_SHAPE, "%s: compact=%d (bit 0: q, bit 1: k)", fn, compact);
    const int base = flags & ~(TF_ATTN_NO_MULTI_V | TF_ATTN_RUN_MULTI_V | TF_ATTN_BANK_ONLY);
    const int part = flags & TF_ATTN_BANK_ONLY;
    if (n_edits == 1)   // today's layout, today's launches (the compact q / k of one edit is the dense one as far as it is read)
        return attn_run_core(fn, q, k, v, out, K, Kq, q_frame0, run_f0, run_n, run, n_runs, S, H, Dh, ld, strides, scale,
                             base | part | (inject_mask ? TF_ATTN_INJECT : 0), dtype, ws, ws_bytes, stream, nullptr);
    if (const int rc = attn_run_check(fn, q, k, v, out, K, Kq, q_frame0, run_f0, run_n, run, n_runs, S, H, Dh, ld, strides,
                                      base | part, dtype, ws, ws_bytes, n_edits))
        return rc;
    const int B = 1 + 2 * n_edits;
    const bool do_src = !part;
    int inj_e[TF_MAX_EDITS], non_e[TF_MAX_EDITS], n_inj = 0, n_non = 0;   // the injecting / the other edits, ascending
    int c_sh[TF_MAX_EDITS];   // compact q / k: slots in front of edit e's uncond slot, minus 1 (an injecting edit reads slot 0)
    for (int e = 0; e < n_edits; ++e) {
        c_sh[e] = 2 * n_non;
        ((inject_mask >> e) & 1u) ? inj_e[n_inj++] = e : non_e[n_non++] = e;
    }
    const RunsLayout L = runs_layout(K, Kq, S, H, Dh, n_runs, n_edits);
    unsigned char* const w8 = static_cast<unsigned char*>(ws);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    {   // the pre-pass: the run's frames of branches [b_lo, B); it also leaves the slots this run fills per injection state
        auto slots = [&](bool inj) {
            const int ns = split_plan(run_n, Kq, S, H, Dh, inj, part, !(flags & TF_ATTN_NO_SPLIT));
            return ns < L.spr ? ns : L.spr;
        };
        AttnParams p{};
        p.k = static_cast<const unsigned char*>(k) + (int64_t)run_f0 * strides[3] * 2;
        const void* v_run = static_cast<const unsigned char*>(v) + (int64_t)run_f0 * strides[5] * 2;
        p.vt = w8 + (size_t)run_f0 * L.Spad * 2;
        p.knorm2 = reinterpret_cast<const float*>(w8 + L.knorm_off) + (size_t)run_f0 * (L.Spad / 64);
        p.K = run_n, p.Kb = K, p.S = S, p.H = H, p.Spad = L.Spad;
        p.ld = ld, p.k_bs = strides[2], p.k_fs = strides[3], p.v_bs = strides[4], p.v_fs = strides[5];
        p.run_hdr = reinterpret_cast<int*>(w8 + L.hdr_off) + run;
        p.nseg = slots(false) | (slots(true) << 16);
        unsigned own = do_src ? 1u : 0u;
        for (int i = 0; i < n_non; ++i) own |= 3u << (1 + 2 * non_e[i]);
        const int b_src = (!do_src && n_inj) ? 1 + 2 * inj_e[0] : -1;
        const unsigned kc_mask = (compact & 2) ? inject_mask : 0u;
        const int b_lo = do_src ? 0 : 1;
        const int rc = dtype == TF_BF16 ? launch_vt_pack<BF16>(p, v_run, Dh, b_lo, B, own, b_src, st, kc_mask)
                                        : launch_vt_pack<F16>(p, v_run, Dh, b_lo, B, own, b_src, st, kc_mask);
        if (rc) return rc;
    }
    const int64_t osz = (flags & TF_ATTN_OUT_F32) ? 4 : 2;
    auto at = [](const void* ptr, int64_t elems, int64_t esz) {
        return static_cast<const void*>(static_cast<const unsigned char*>(ptr) + elems * esz);
    };
    auto call = [&](int e, int fl, const RunEditsPart& ed) {   // the bank branches of edit e (of a pair from e on) / the source branch
        const bool src = ed.src_only != 0;
        const int sh = src ? 0 : 2 * e;
        const bool own_qk = !src && !(fl & TF_ATTN_INJECT);
        const int qsh = own_qk ? ((compact & 1) ? c_sh[e] : 2 * e) : 0, ksh = own_qk ? ((compact & 2) ? c_sh[e] : 2 * e) : 0;
        return attn_run_core(fn, at(q, qsh * strides[0], 2), at(k, ksh * strides[2], 2), at(v, sh * strides[4], 2),
                             const_cast<void*>(at(out, sh * strides[6], osz)), K, Kq, q_frame0, run_f0, run_n, run, n_runs, S, H,
                             Dh, ld, strides, scale, fl, dtype, ws, ws_bytes, stream, &ed);
    };
    // the four-bank form of a run (TF_ATTN_RUN_MULTI_V): Dh = 40 or 64, fp32 score scaling, at least one pair of INJECTING edits
    const bool mv = (flags & TF_ATTN_RUN_MULTI_V) && !(flags & (TF_ATTN_NO_MULTI_V | TF_ATTN_FOLD_SCALE)) && (Dh == 40 || Dh == 64) &&
                    n_inj >= 2;
    // bank branches first (the long problems): the injecting edits (pairs in the four-bank form, an odd last one in its own
    // launches), then the others; then the source branch
    int i = 0;
    if (mv)
        for (; i + 2 <= n_inj; i += 2)
            if (const int rc = call(inj_e[i], base | TF_ATTN_INJECT | TF_ATTN_BANK_ONLY,
                                    RunEditsPart::pair_mv4(n_edits, inj_e[i], inj_e[i + 1])))
                return rc;
    for (; i < n_inj; ++i)
        if (const int rc = call(inj_e[i], base | TF_ATTN_INJECT | TF_ATTN_BANK_ONLY, RunEditsPart::bank(n_edits, inj_e[i])))
            return rc;
    for (i = 0; i < n_non; ++i)
        if (const int rc = call(non_e[i], base | TF_ATTN_BANK_ONLY, RunEditsPart::bank(n_edits, non_e[i]))) return rc;
    // (the source launch sees TF_ATTN_INJECT iff every edit injects, as in the one-call form: its result does not depend on it)
    return do_src ? call(0, base | (n_non == 0 ? TF_ATTN_INJECT : 0), RunEditsPart::source(n_edits)) : 0;
}

extern "C" int tf_ext_attn_runs_merge_edits(void* out, int K, int Kq, int S, int H, int Dh, int n_runs, int n_edits,
                                            unsigned inject_mask, int64_t out_branch_stride, int64_t out_frame_stride,
                                            int flags, int dtype, void* ws, size_t ws_bytes, void* stream) {
    const char* const fn = "tf_ext_attn_runs_merge_edits";
    if (const int rc = run_edits_check(fn, n_edits, inject_mask, flags)) return rc;
    return attn_runs_merge_core(fn, out, K, Kq, S, H, Dh, n_runs, n_edits, inject_mask, out_branch_stride, out_frame_stride,
                                flags, dtype, ws, ws_bytes, stream);
}

// Launch plan of ONE run call over run_n of the bank's K frames (dense tensors, the run and the query frames at frame 0)
// followed by the merge of n_runs runs, recorded by the entry points themselves as tf_ext_attn_plan does.
extern "C" int tf_ext_attn_run_plan(int K, int Kq, int run_n, int n_runs, int S, int H, int Dh, int flags, int dtype, char* buf,
                                    size_t len) {
    if (const int rc = runs_check_shape("tf_ext_attn_run_plan", K, Kq, S, H, Dh, n_runs, dtype)) return rc;
    void* const ph = reinterpret_cast<void*>((uintptr_t)1 << 12);
    const int64_t ld = (int64_t)H * Dh, fs = (int64_t)S * ld;
    const int64_t strides[9] = {Kq * fs, fs, K * fs, fs, K * fs, fs, Kq * fs, fs, ld};
    const size_t wsb = tf_ext_attn_runs_workspace_bytes(K, Kq, S, H, Dh, n_runs, dtype);
    TfPlanRec rec{buf, len, 0, 0};
    if (buf && len) buf[0] = 0;
    tf_plan_rec = &rec;
    int rc = tf_ext_attn_run(ph, ph, ph, ph, K, Kq, 0, 0, run_n, 0, n_runs, S, H, Dh, ld, strides, 1.0f, flags, dtype, ph, wsb,
                             nullptr);
    if (!rc) rc = tf_ext_attn_runs_merge(ph, K, Kq, S, H, Dh, n_runs, Kq * fs, fs, flags, dtype, ph, wsb, nullptr);
    tf_plan_rec = nullptr;
    if (rc) return rc;
    TF_ARG(rec.used < len, TF_ERR_WORKSPACE, "tf_ext_attn_run_plan: the plan needs %zu bytes", rec.used + 1);
    return rec.n;
}

// The same for ONE tf_ext_attn_run_edits call followed by tf_ext_attn_runs_merge_edits.
extern "C" int tf_ext_attn_run_edits_plan(int K, int Kq, int run_n, int n_runs, int S, int H, int Dh, int n_edits,
                                          unsigned inject_mask, int flags, int dtype, char* buf, size_t len) {
    if (const int rc = run_edits_check("tf_ext_attn_run_edits_plan", n_edits, inject_mask, flags)) return rc;
    if (const int rc = runs_check_shape("tf_ext_attn_run_edits_plan", K, Kq, S, H, Dh, n_runs, dtype)) return rc;
    void* const ph = reinterpret_cast<void*>((uintptr_t)1 << 12);
    const int64_t ld = (int64_t)H * Dh, fs = (int64_t)S * ld;
    const int64_t strides[9] = {Kq * fs, fs, K * fs, fs, K * fs, fs, Kq * fs, fs, ld};
    const size_t wsb = tf_ext_attn_runs_edits_workspace_bytes(K, Kq, S, H, Dh, n_runs, n_edits, dtype);
    TfPlanRec rec{buf, len, 0, 0};
    if (buf && len) buf[0] = 0;
    tf_plan_rec = &rec;
    int rc = tf_ext_attn_run_edits(ph, ph, ph, ph, K, Kq, 0, 0, run_n, 0, n_runs, S, H, Dh, ld, strides, 1.0f, flags, dtype,
                                   n_edits, inject_mask, 0, ph, wsb, nullptr);
    if (!rc)
        rc = tf_ext_attn_runs_merge_edits(ph, K, Kq, S, H, Dh, n_runs, n_edits, inject_mask, Kq * fs, fs, flags, dtype, ph, wsb,
                                          nullptr);
    tf_plan_rec = nullptr;
    if (rc) return rc;
    TF_ARG(rec.used < len, TF_ERR_WORKSPACE, "tf_ext_attn_run_edits_plan: the plan needs %zu bytes", rec.used + 1);
    return rec.n;
}

// Launch plan of tf_ext_attn_fwd for dense tensors (ld = H*Dh): the entry point itself runs under the plan recorder
// (csrc/tf_common.h), so the fused-kernel decision, the split plan and the kernel choice are the ones a real call makes.
// The pointers it is given are placeholders: every launch is recorded instead of issued, nothing is dereferenced.
extern "C" int tf_ext_attn_plan(int K, int Kq, int S, int H, int Dh, int flags, int dtype, char* buf, size_t len) {
    TF_ARG(K > 0 && S > 0 && H > 0 && Kq > 0 && Kq <= K, TF_ERR_SHAPE, "tf_ext_attn_plan: K=%d Kq=%d S=%d H=%d", K, Kq, S,
           H);
    void* const ph = reinterpret_cast<void*>((uintptr_t)1 << 12);
    const int64_t ld = (int64_t)H * Dh, fs = (int64_t)S * ld;
    const int64_t strides[9] = {Kq * fs, fs, K * fs, fs, K * fs, fs, Kq * fs, fs, ld};
    TfPlanRec rec{buf, len, 0, 0};
    if (buf && len) buf[0] = 0;
    tf_plan_rec = &rec;
    const int rc = tf_ext_attn_fwd_strided(ph, ph, ph, ph, K, Kq, 0, S, H, Dh, ld, strides, 1.0f, flags,
                                           dtype, ph, tf_ext_attn_workspace_bytes(K, S, H, Dh, dtype), nullptr);
    tf_plan_rec = nullptr;
    if (rc) return rc;
    TF_ARG(rec.used < len, TF_ERR_WORKSPACE, "tf_ext_attn_plan: the plan needs %zu bytes", rec.used + 1);
    return rec.n;
}

extern "C" int tf_ext_attn_fwd(const void* q, const void* k, const void* v, void* out, int K, int Kq, int q_frame0,
                               int S, int H, int Dh, int64_t ld, float scale, int inject, int dtype, void* ws,
                               size_t ws_bytes, void* stream) {
    // dense [3, frames, S, ld] tensors; out [3, Kq, S, H*Dh]
    const int64_t fs = (int64_t)S * ld, ofs = (int64_t)S * H * Dh;
    const int64_t strides[9] = {Kq * fs, fs, K * fs, fs, K * fs, fs, Kq * ofs, ofs, ld};
    return tf_ext_attn_fwd_strided(q, k, v, out, K, Kq, q_frame0, S, H, Dh, ld, strides, scale, inject, dtype, ws,
                                   ws_bytes, stream);
}

// ---------------------------------------------------------------------------------------------
// Keyframe segments (include/tokenflow_hip.h): a pass of V scenes or clips, segment v = K_v consecutive keyframes of the bank.
// Every segment is the single-clip call on its own frame window; the composition shares the launches that can be shared -- ONE
// fused multi-set launch for the segments whose own call is fused, ONE V^T pre-pass for the ones that stream.
extern "C" size_t tf_ext_attn_segments_workspace_bytes(int K, int S, int H, int Dh, int dtype) {
    return attn_seg_ws_bytes(K, S, H, Dh, dtype);
}

extern "C" int tf_ext_attn_fwd_segments(const void* q, const void* k, const void* v, void* out, int K, int n_seg,
                                        const int* seg_K, int S, int H, int Dh, int64_t ld, float scale, int flags, int dtype,
                                        void* ws, size_t ws_bytes, void* stream) {
    const char* const name = "tf_ext_attn_fwd_segments";
    TF_ARG(seg_K, TF_ERR_NULL, "%s: null seg_K", name);
    TF_ARG(n_seg >= 1 && n_seg <= TF_MAX_SEGMENTS, TF_ERR_SHAPE, "%s: n_seg=%d (1 .. %d)", name, n_seg, TF_MAX_SEGMENTS);
    int sum = 0;
    for (int i = 0; i < n_seg; ++i) {
        TF_ARG(seg_K[i] >= 1 && seg_K[i] <= K, TF_ERR_SHAPE, "%s: segment %d has %d keyframes (1 .. K = %d)", name, i, seg_K[i], K);
        sum += seg_K[i];
    }
    TF_ARG(sum == K, TF_ERR_SHAPE, "%s: the segments hold %d keyframes, the pass %d", name, sum, K);
    constexpr int REFUSED = TF_ATTN_BANK_ONLY | TF_ATTN_SOURCE_ONLY | TF_ATTN_MULTI_V | TF_ATTN_NO_MULTI_V | TF_ATTN_MULTI_V64 |
                            TF_ATTN_RUN_MULTI_V;
    TF_ARG(!(flags & REFUSED), TF_ERR_SHAPE,
           "%s: flags 0x%x -- TF_ATTN_BANK_ONLY / TF_ATTN_SOURCE_ONLY and the multi-edit hints have no segment form", name,
           flags & REFUSED);
    if (n_seg == 1)   // one shot: today's call
        return tf_ext_attn_fwd(q, k, v, out, K, K, 0, S, H, Dh, ld, scale, flags, dtype, ws, ws_bytes, stream);
    TF_ARG(q && k && v && out && ws, TF_ERR_NULL, "%s: null pointer", name);
    TF_ARG(dtype == TF_BF16 || dtype == TF_F16, TF_ERR_DTYPE, "%s: dtype %d (bf16/f16 only)", name, dtype);
    TF_ARG(S > 0 && H > 0 && (Dh == 40 || Dh == 64 || Dh == 80 || Dh == 160) && ld >= (int64_t)H * Dh && ld % 8 == 0, TF_ERR_SHAPE,
           "%s: S=%d H=%d Dh=%d ld=%lld", name, S, H, Dh, (long long)ld);
    TF_ARG(ws_bytes >= attn_seg_ws_bytes(K, S, H, Dh, dtype), TF_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", name, ws_bytes,
           attn_seg_ws_bytes(K, S, H, Dh, dtype));
    // dense [3, K, S, ld] tensors, out [3, K, S, H*Dh]: a segment keeps the pass's branch strides
    const int64_t fs = (int64_t)S * ld, ofs = (int64_t)S * H * Dh;
    const int64_t strides[9] = {K * fs, fs, K * fs, fs, K * fs, fs, K * ofs, ofs, ld};
    const int64_t osz = (flags & TF_ATTN_OUT_F32) ? 4 : 2;
    auto at = [](const void* ptr, int64_t elems, int64_t esz) {
        return static_cast<const void*>(static_cast<const unsigned char*>(ptr) + elems * esz);
    };
    int f0[TF_MAX_SEGMENTS], fused[TF_MAX_SEGMENTS], n_fused = 0;
    auto call = [&](int i, int fl, int probe) {   // segment i's own call on its frame window
        const SegPart sg{K, f0[i], probe};
        return attn_fwd_core(at(q, f0[i] * fs, 2), at(k, f0[i] * fs, 2), at(v, f0[i] * fs, 2),
                             const_cast<void*>(at(out, f0[i] * ofs, osz)), seg_K[i], seg_K[i], 0, S, H, Dh, ld, strides, scale, fl,
                             dtype, ws, ws_bytes, stream, nullptr, &sg);
    };
    for (int i = 0, f = 0; i < n_seg; f += seg_K[i++]) {
        f0[i] = f;
        fused[i] = call(i, flags, 1);   // the decision of the segment's own call
        if (fused[i] < 0) return fused[i];
        n_fused += fused[i];
    }
    bool joint = false;
    TfAttnSet sets[TF_MAX_SEGMENTS] = {};
    TfFusedPlan plan{};
    if (n_fused) {   // ONE launch, a tensor set per fused segment -- where the plan of the joint grid stays in the fused range
        int n = 0;
        for (int i = 0; i < n_seg; ++i) {
            if (!fused[i]) continue;
            TfAttnSet& a = sets[n++];
            a.q = at(q, f0[i] * fs, 2), a.k = at(k, f0[i] * fs, 2), a.v = at(v, f0[i] * fs, 2);
            a.out = const_cast<void*>(at(out, f0[i] * ofs, osz));
            a.q_bs = strides[0], a.q_fs = strides[1], a.ld_q = ld;
            a.k_bs = strides[2], a.k_fs = strides[3], a.v_bs = strides[4], a.v_fs = strides[5], a.ld = ld;
            a.o_bs = strides[6], a.o_fs = strides[7];
            a.H = H, a.Kq = a.Kb = seg_K[i], a.q_frame0 = 0, a.b0 = 0, a.nb = 3;
        }
        plan = tf_attn_fused_plan(sets, n_fused, S, Dh, dtype, flags);
        joint = plan.use != 0;
    }
    // where the joint grid leaves the fused range (the default mode decides per grid, as a one-shot call of that size would),
    // those segments stream beside the others
    const int stream_flags = flags | (n_fused && !joint ? TF_ATTN_NO_FUSED : 0);
    if (!joint || n_fused < n_seg) {
        // ONE pre-pass over the whole bank: every branch, the key norms as the single-clip call leaves them
        const int Spad = ((S + 127) / 128) * 128;
        const bool inj = (flags & TF_ATTN_INJECT) != 0;
        AttnParams p{};
        p.k = k, p.vt = ws;
        p.knorm2 = reinterpret_cast<const float*>(static_cast<unsigned char*>(ws) + ((vt_bytes(K, Spad, H, Dh, 3) + 255) & ~(size_t)255));
        p.K = p.Kb = K, p.S = S, p.H = H, p.Spad = Spad, p.nseg = 1;
        p.ld = ld, p.k_bs = strides[2], p.k_fs = strides[3], p.v_bs = strides[4], p.v_fs = strides[5];
        hipStream_t st = reinterpret_cast<hipStream_t>(stream);
        const int rc = dtype == TF_BF16 ? launch_vt_pack<BF16>(p, v, Dh, 0, 3, inj ? 0u : ~0u, inj ? 0 : -1, st)
                                        : launch_vt_pack<F16>(p, v, Dh, 0, 3, inj ? 0u : ~0u, inj ? 0 : -1, st);
        if (rc) return rc;
        for (int i = 0; i < n_seg; ++i)
            if (!joint || !fused[i])
                if (const int rc2 = call(i, stream_flags, 0)) return rc2;
    }
    if (!joint) return 0;
    tf_plan_sets_note = 1;   // the plan token of this launch names its sets whatever their number
    const int rc = tf_attn_fused_launch(sets, n_fused, S, Dh, scale, flags, dtype, plan, reinterpret_cast<hipStream_t>(stream));
    tf_plan_sets_note = 0;
    return rc;
}

// Launch plan of tf_ext_attn_fwd_segments (host only): the entry point itself under the plan recorder.
extern "C" int tf_ext_attn_segments_plan(int K, int n_seg, const int* seg_K, int S, int H, int Dh, int flags, int dtype,
                                         char* buf, size_t len) {
    TF_ARG(K > 0 && S > 0 && H > 0, TF_ERR_SHAPE, "tf_ext_attn_segments_plan: K=%d S=%d H=%d", K, S, H);
    void* const ph = reinterpret_cast<void*>((uintptr_t)1 << 12);
    TfPlanRec rec{buf, len, 0, 0};
    if (buf && len) buf[0] = 0;
    tf_plan_rec = &rec;
    const int rc = tf_ext_attn_fwd_segments(ph, ph, ph, ph, K, n_seg, seg_K, S, H, Dh, (int64_t)H * Dh, 1.0f, flags, dtype, ph,
                                            (size_t)-1, nullptr);
    tf_plan_rec = nullptr;
    if (rc) return rc;
    TF_ARG(rec.used < len, TF_ERR_WORKSPACE, "tf_ext_attn_segments_plan: the plan needs %zu bytes", rec.used + 1);
    return rec.n;
}

// ---------------------------------------------------------------------------------------------
// Sliding-window keyframe bank (include/tokenflow_hip.h): the uncond / cond branches of query frame i attend to the keys of
// bank frames [win_lo[i], win_lo[i] + win_n[i]) only.  The launches of tf_ext_attn_fwd_strided for a bank of max_i win_n[i]
// frames -- ONE pre-pass over the whole bank, ONE bank launch whose problems decode their frame's window from the table in the
// kernel arguments -- so frame i's result is what its own call (the strided call on its window alone) computes.
// The window table of a call, validated and packed as the kernels read it.
static int windows_pack(const char* name, int K, int Kq, int q_frame0, const int* win_lo, const int* win_n, unsigned* win,
                        int* K_max, bool* full) {
    TF_ARG(win_lo && win_n, TF_ERR_NULL, "%s: null window table", name);
    TF_ARG(K > 0 && Kq > 0 && q_frame0 >= 0 && q_frame0 + Kq <= K, TF_ERR_SHAPE,
           "%s: query frames [%d, %d) outside the %d-frame bank", name, q_frame0, q_frame0 + Kq, K);
    TF_ARG(Kq <= TF_MAX_WINDOW_FRAMES, TF_ERR_SHAPE, "%s: Kq=%d (at most %d query frames carry a window)", name, Kq,
           TF_MAX_WINDOW_FRAMES);
    *K_max = 0, *full = true;
    for (int i = 0; i < Kq; ++i) {
        const int lo = win_lo[i], n = win_n[i], own = q_frame0 + i;
        TF_ARG(n >= 1, TF_ERR_SHAPE, "%s: window %d holds %d frames", name, i, n);
        TF_ARG(lo >= 0 && lo <= K - n && K < (1 << 16), TF_ERR_SHAPE, "%s: window %d = [%d, %d) outside the %d-frame bank", name, i,
               lo, lo + n, K);
        TF_ARG(lo <= own && own < lo + n, TF_ERR_SHAPE, "%s: window %d = [%d, %d) does not hold its own frame %d", name, i, lo,
               lo + n, own);
        win[i] = (unsigned)lo | ((unsigned)n << 16);
        *K_max = n > *K_max ? n : *K_max;
        *full = *full && lo == 0 && n == K;
    }
    return 0;
}

// The flags no windowed call has; tf_ext_attn_fwd_windows refuses the part flags too.
constexpr int WIN_REFUSED = TF_ATTN_FOLD_SCALE | TF_ATTN_MULTI_V | TF_ATTN_NO_MULTI_V | TF_ATTN_MULTI_V64 | TF_ATTN_RUN_MULTI_V;

// tf_ext_attn_fwd_windows and tf_ext_attn_fwd_windows_part: the two differ in the flags they refuse (and in how they say so).
static int windows_fwd(const char* name, int refused, const char* refused_what, const void* q, const void* k, const void* v,
                       void* out, int K, int Kq, int q_frame0, int S, int H, int Dh, int64_t ld, const int64_t* strides,
                       float scale, int flags, int dtype, const int* win_lo, const int* win_n, void* ws, size_t ws_bytes,
                       void* stream) {
    unsigned win[TF_MAX_WINDOW_FRAMES];
    int K_max = 0;
    bool full = true;
    if (const int rc = windows_pack(name, K, Kq, q_frame0, win_lo, win_n, win, &K_max, &full)) return rc;
    TF_ARG(!(flags & refused), TF_ERR_SHAPE, "%s: flags 0x%x -- %s", name, flags & refused, refused_what);
    if (full)   // every keyframe sees the whole bank: today's call (with the same part flag, if any)
        return tf_ext_attn_fwd_strided(q, k, v, out, K, Kq, q_frame0, S, H, Dh, ld, strides, scale, flags, dtype, ws, ws_bytes,
                                       stream);
    const WinPart wn{win, K_max};
    return attn_fwd_core(q, k, v, out, K, Kq, q_frame0, S, H, Dh, ld, strides, scale, flags, dtype, ws, ws_bytes, stream, nullptr,
                         nullptr, &wn);
}

// The launch plan of either entry point for dense tensors (host only): the entry point itself under the plan recorder.
template <typename Fn>
static int windows_plan(const char* name, Fn fwd, int K, int Kq, int q_frame0, int S, int H, int Dh, int flags, int dtype,
                        const int* win_lo, const int* win_n, char* buf, size_t len) {
    TF_ARG(K > 0 && S > 0 && H > 0 && Kq > 0 && Kq <= K, TF_ERR_SHAPE, "%s: K=%d Kq=%d S=%d H=%d", name, K, Kq, S, H);
    void* const ph = reinterpret_cast<void*>((uintptr_t)1 << 12);
    const int64_t ld = (int64_t)H * Dh, fs = (int64_t)S * ld;
    const int64_t strides[9] = {Kq * fs, fs, K * fs, fs, K * fs, fs, Kq * fs, fs, ld};
    TfPlanRec rec{buf, len, 0, 0};
    if (buf && len) buf[0] = 0;
    tf_plan_rec = &rec;
    const int rc = fwd(ph, ph, ph, ph, K, Kq, q_frame0, S, H, Dh, ld, strides, 1.0f, flags, dtype, win_lo, win_n, ph,
                       tf_ext_attn_workspace_bytes(K, S, H, Dh, dtype), nullptr);
    tf_plan_rec = nullptr;
    if (rc) return rc;
    TF_ARG(rec.used < len, TF_ERR_WORKSPACE, "%s: the plan needs %zu bytes", name, rec.used + 1);
    return rec.n;
}

extern "C" int tf_ext_attn_fwd_windows(const void* q, const void* k, const void* v, void* out, int K, int Kq, int q_frame0,
                                       int S, int H, int Dh, int64_t ld, const int64_t* strides, float scale, int flags,
                                       int dtype, const int* win_lo, const int* win_n, void* ws, size_t ws_bytes,
                                       void* stream) {
    return windows_fwd("tf_ext_attn_fwd_windows", WIN_REFUSED | TF_ATTN_BANK_ONLY | TF_ATTN_SOURCE_ONLY,
                       "TF_ATTN_BANK_ONLY / TF_ATTN_SOURCE_ONLY / TF_ATTN_FOLD_SCALE and the multi-edit hints have no windowed form",
                       q, k, v, out, K, Kq, q_frame0, S, H, Dh, ld, strides, scale, flags, dtype, win_lo, win_n, ws, ws_bytes,
                       stream);
}

// The bank part of a windowed pass (include/tokenflow_hip.h): tf_ext_attn_fwd_windows with TF_ATTN_BANK_ONLY accepted -- k and v
// hold only the slabs the bank branches read, addressed as in tf_ext_attn_fwd_strided with that flag.  What a frame-sharded rank
// runs over its halo-extended receive buffer; the source part of a windowed pass is window-free (tf_ext_attn_fwd_strided with
// TF_ATTN_SOURCE_ONLY).
extern "C" int tf_ext_attn_fwd_windows_part(const void* q, const void* k, const void* v, void* out, int K, int Kq, int q_frame0,
                                            int S, int H, int Dh, int64_t ld, const int64_t* strides, float scale, int flags,
                                            int dtype, const int* win_lo, const int* win_n, void* ws, size_t ws_bytes,
                                            void* stream) {
    return windows_fwd("tf_ext_attn_fwd_windows_part", WIN_REFUSED | TF_ATTN_SOURCE_ONLY,
                       "TF_ATTN_SOURCE_ONLY (the source part of a windowed pass is tf_ext_attn_fwd_strided) / TF_ATTN_FOLD_SCALE "
                       "and the multi-edit hints have no windowed form",
                       q, k, v, out, K, Kq, q_frame0, S, H, Dh, ld, strides, scale, flags, dtype, win_lo, win_n, ws, ws_bytes,
                       stream);
}

extern "C" int tf_ext_attn_windows_part_plan(int K, int Kq, int q_frame0, int S, int H, int Dh, int flags, int dtype,
                                             const int* win_lo, const int* win_n, char* buf, size_t len) {
    return windows_plan("tf_ext_attn_windows_part_plan", tf_ext_attn_fwd_windows_part, K, Kq, q_frame0, S, H, Dh, flags, dtype,
                        win_lo, win_n, buf, len);
}

extern "C" int tf_ext_attn_windows_plan(int K, int Kq, int q_frame0, int S, int H, int Dh, int flags, int dtype,
                                        const int* win_lo, const int* win_n, char* buf, size_t len) {
    return windows_plan("tf_ext_attn_windows_plan", tf_ext_attn_fwd_windows, K, Kq, q_frame0, S, H, Dh, flags, dtype, win_lo,
                        win_n, buf, len);
}

// ---------------------------------------------------------------------------------------------
// Sliding-window bank for a multi-edit batch (include/tokenflow_hip.h): the masked composition with the window table handed to
// every bank part -- ONE pre-pass, the injecting edits (pairs in the windowed four-bank form where it is selected), the others,
// then the plain source-only launches.
extern "C" int tf_ext_attn_fwd_windows_edits(const void* q, const void* k, const void* v, void* out, int K, int Kq, int q_frame0,
                                             int S, int H, int Dh, int64_t ld, const int64_t* strides, float scale, int flags,
                                             int dtype, int n_edits, unsigned inject_mask, const int* win_lo, const int* win_n,
                                             void* ws, size_t ws_bytes, void* stream) {
    const char* const name = "tf_ext_attn_fwd_windows_edits";
    unsigned win[TF_MAX_WINDOW_FRAMES];
    int K_max = 0;
    bool full = true;
    if (const int rc = windows_pack(name, K, Kq, q_frame0, win_lo, win_n, win, &K_max, &full)) return rc;
    // (the multi-edit hints TF_ATTN_MULTI_V / TF_ATTN_NO_MULTI_V / TF_ATTN_MULTI_V64 select the pair form here)
    constexpr int REFUSED = TF_ATTN_BANK_ONLY | TF_ATTN_SOURCE_ONLY | TF_ATTN_FOLD_SCALE | TF_ATTN_RUN_MULTI_V;
    TF_ARG(!(flags & REFUSED), TF_ERR_SHAPE,
           "%s: flags 0x%x -- TF_ATTN_BANK_ONLY / TF_ATTN_SOURCE_ONLY / TF_ATTN_FOLD_SCALE / TF_ATTN_RUN_MULTI_V have no windowed "
           "form", name, flags & REFUSED);
    // (n_edits = 1: the masked composition is attn_fwd_core on today's layout, here with the window table: tf_ext_attn_fwd_windows)
    const WinPart wn{win, K_max};
    // every window = [0, K): the masked call itself
    return attn_fwd_edits_masked(name, q, k, v, out, K, Kq, q_frame0, S, H, Dh, ld, strides, scale, flags, dtype, n_edits,
                                 inject_mask, ws, ws_bytes, stream, false, 0, full ? nullptr : &wn);
}

// Launch plan of tf_ext_attn_fwd_windows_edits for dense tensors (host only): the entry point itself under the plan recorder.
extern "C" int tf_ext_attn_windows_edits_plan(int K, int Kq, int q_frame0, int S, int H, int Dh, int n_edits, unsigned inject_mask,
                                              int flags, int dtype, const int* win_lo, const int* win_n, char* buf, size_t len) {
    TF_ARG(K > 0 && S > 0 && H > 0 && Kq > 0 && Kq <= K, TF_ERR_SHAPE, "tf_ext_attn_windows_edits_plan: K=%d Kq=%d S=%d H=%d", K,
           Kq, S, H);
    void* const ph = reinterpret_cast<void*>((uintptr_t)1 << 12);
    const int64_t ld = (int64_t)H * Dh, fs = (int64_t)S * ld;
    const int64_t strides[9] = {Kq * fs, fs, K * fs, fs, K * fs, fs, Kq * fs, fs, ld};
    TfPlanRec rec{buf, len, 0, 0};
    if (buf && len) buf[0] = 0;
    tf_plan_rec = &rec;
    const int rc = tf_ext_attn_fwd_windows_edits(ph, ph, ph, ph, K, Kq, q_frame0, S, H, Dh, ld, strides, 1.0f, flags, dtype, n_edits,
                                                 inject_mask, win_lo, win_n, ph, (size_t)-1, nullptr);
    tf_plan_rec = nullptr;
    if (rc) return rc;
    TF_ARG(rec.used < len, TF_ERR_WORKSPACE, "tf_ext_attn_windows_edits_plan: the plan needs %zu bytes", rec.used + 1);
    return rec.n;
}

// The bank part of a windowed multi-edit pass (include/tokenflow_hip.h): tf_ext_attn_fwd_windows_edits with TF_ATTN_BANK_ONLY
// accepted and q / k dense or compact as in tf_ext_attn_fwd_edits_part -- what a frame-sharded rank would run over its
// halo-extended receive buffer for all E edits at once.  The masked composition as a part call with the window table: where every
// edit's bank part takes the fused small-problem kernel they share ONE launch under the one table (fused[..,sets=E,win]); the
// streaming regime is the composition of tf_ext_attn_fwd_windows_edits without its source launches.  The source part of a
// windowed pass is window-free: tf_ext_attn_fwd_edits_part(TF_ATTN_SOURCE_ONLY).
extern "C" int tf_ext_attn_fwd_windows_edits_part(const void* q, const void* k, const void* v, void* out, int K, int Kq,
                                                  int q_frame0, int S, int H, int Dh, int64_t ld, const int64_t* strides,
                                                  float scale, int flags, int dtype, int n_edits, unsigned inject_mask,
                                                  int qk_compact, const int* win_lo, const int* win_n, void* ws, size_t ws_bytes,
                                                  void* stream) {
    const char* const name = "tf_ext_attn_fwd_windows_edits_part";
    TF_ARG(qk_compact == 0 || qk_compact == 1, TF_ERR_SHAPE, "%s: qk_compact=%d (0 or 1)", name, qk_compact);
    if (!(flags & TF_ATTN_BANK_ONLY)) {   // without the flag the call IS tf_ext_attn_fwd_windows_edits (which refuses the source flag)
        TF_ARG(!qk_compact || (flags & TF_ATTN_SOURCE_ONLY), TF_ERR_SHAPE,
               "%s: qk_compact=1 without TF_ATTN_BANK_ONLY (the whole call reads dense q / k)", name);
        return tf_ext_attn_fwd_windows_edits(q, k, v, out, K, Kq, q_frame0, S, H, Dh, ld, strides, scale, flags, dtype, n_edits,
                                             inject_mask, win_lo, win_n, ws, ws_bytes, stream);
    }
    unsigned win[TF_MAX_WINDOW_FRAMES];
    int K_max = 0;
    bool full = true;
    if (const int rc = windows_pack(name, K, Kq, q_frame0, win_lo, win_n, win, &K_max, &full)) return rc;
    constexpr int REFUSED = TF_ATTN_SOURCE_ONLY | TF_ATTN_FOLD_SCALE | TF_ATTN_RUN_MULTI_V;
    TF_ARG(!(flags & REFUSED), TF_ERR_SHAPE,
           "%s: flags 0x%x -- TF_ATTN_SOURCE_ONLY (the source part of a windowed pass is tf_ext_attn_fwd_edits_part) / "
           "TF_ATTN_FOLD_SCALE / TF_ATTN_RUN_MULTI_V have no windowed form", name, flags & REFUSED);
    // (n_edits = 1: the masked composition is attn_fwd_core with the part flag and the window table: tf_ext_attn_fwd_windows_part)
    const WinPart wn{win, K_max};
    // every window = [0, K): tf_ext_attn_fwd_edits_part itself
    return attn_fwd_edits_masked(name, q, k, v, out, K, Kq, q_frame0, S, H, Dh, ld, strides, scale, flags, dtype, n_edits,
                                 inject_mask, ws, ws_bytes, stream, true, qk_compact, full ? nullptr : &wn);
}

// Launch plan of tf_ext_attn_fwd_windows_edits_part for dense tensors (q / k dense or compact: the plan does not depend on it).
extern "C" int tf_ext_attn_windows_edits_part_plan(int K, int Kq, int q_frame0, int S, int H, int Dh, int n_edits,
                                                   unsigned inject_mask, int qk_compact, int flags, int dtype, const int* win_lo,
                                                   const int* win_n, char* buf, size_t len) {
    TF_ARG(K > 0 && S > 0 && H > 0 && Kq > 0 && Kq <= K, TF_ERR_SHAPE, "tf_ext_attn_windows_edits_part_plan: K=%d Kq=%d S=%d H=%d",
           K, Kq, S, H);
    void* const ph = reinterpret_cast<void*>((uintptr_t)1 << 12);
    const int64_t ld = (int64_t)H * Dh, fs = (int64_t)S * ld;
    const int64_t strides[9] = {Kq * fs, fs, K * fs, fs, K * fs, fs, Kq * fs, fs, ld};
    TfPlanRec rec{buf, len, 0, 0};
    if (buf && len) buf[0] = 0;
    tf_plan_rec = &rec;
    const int rc = tf_ext_attn_fwd_windows_edits_part(ph, ph, ph, ph, K, Kq, q_frame0, S, H, Dh, ld, strides, 1.0f, flags, dtype,
                                                      n_edits, inject_mask, qk_compact, win_lo, win_n, ph, (size_t)-1, nullptr);
    tf_plan_rec = nullptr;
    if (rc) return rc;
    TF_ARG(rec.used < len, TF_ERR_WORKSPACE, "tf_ext_attn_windows_edits_part_plan: the plan needs %zu bytes", rec.used + 1);
    return rec.n;
}

// ---------------------------------------------------------------------------------------------
// Frame-set keyframe bank (include/tokenflow_hip.h): the uncond / cond branches of query frame i attend to the keys of the bank
// frames whose bits are set in sets[i], in ascending frame order.  A table of contiguous ranges IS tf_ext_attn_fwd_windows on
// the equivalent (lo, n) table (and so tf_ext_attn_fwd_strided when every set is the whole bank): delegated here, so those paths
// are reached unchanged.  Everything else: the launches of tf_ext_attn_fwd_strided for a bank of max_i popcount(sets[i]) frames
// -- ONE pre-pass over the whole bank, ONE bank launch whose problems walk their frame's member mask from the table in the
// kernel arguments -- so frame i's result is what its own call (the strided call on its member frames, gathered) computes.
//
// The set table of a call (this one's and tf_ext_attn_fwd_frame_sets_edits'), validated: the equivalent (lo, n) table, the largest set, and whether every set is a contiguous range.
static int frame_sets_check(const char* name, int K, int Kq, int q_frame0, const uint64_t* sets, int* win_lo, int* win_n,
                            int* K_max, bool* ranges) {
    TF_ARG(sets, TF_ERR_NULL, "%s: null set table", name);
    TF_ARG(K > 0 && Kq > 0 && q_frame0 >= 0 && q_frame0 + Kq <= K, TF_ERR_SHAPE,
           "%s: query frames [%d, %d) outside the %d-frame bank", name, q_frame0, q_frame0 + Kq, K);
    TF_ARG(K <= 64, TF_ERR_SHAPE, "%s: K=%d (a set is a 64-bit mask: at most 64 bank frames)", name, K);
    TF_ARG(Kq <= TF_MAX_WINDOW_FRAMES, TF_ERR_SHAPE, "%s: Kq=%d (at most %d query frames carry a set)", name, Kq,
           TF_MAX_WINDOW_FRAMES);
    *K_max = 0, *ranges = true;
    for (int i = 0; i < Kq; ++i) {
        const uint64_t m = sets[i];
        const int own = q_frame0 + i;
        TF_ARG(m != 0, TF_ERR_SHAPE, "%s: set %d is empty", name, i);
        TF_ARG(K == 64 || !(m >> K), TF_ERR_SHAPE, "%s: set %d = 0x%llx has bits at or above the %d-frame bank", name, i,
               (unsigned long long)m, K);
        TF_ARG((m >> own) & 1u, TF_ERR_SHAPE, "%s: set %d = 0x%llx does not hold its own frame %d", name, i, (unsigned long long)m,
               own);
        const int lo = __builtin_ctzll(m), n = __builtin_popcountll(m);
        win_lo[i] = lo, win_n[i] = n;
        *ranges = *ranges && (m >> lo) == (n == 64 ? ~(uint64_t)0 : ((uint64_t)1 << n) - 1);
        *K_max = n > *K_max ? n : *K_max;
    }
    return 0;
}

extern "C" int tf_ext_attn_fwd_frame_sets(const void* q, const void* k, const void* v, void* out, int K, int Kq, int q_frame0,
                                          int S, int H, int Dh, int64_t ld, const int64_t* strides, float scale, int flags,
                                          int dtype, const uint64_t* sets, void* ws, size_t ws_bytes, void* stream) {
    const char* const name = "tf_ext_attn_fwd_frame_sets";
    int win_lo[TF_MAX_WINDOW_FRAMES], win_n[TF_MAX_WINDOW_FRAMES], K_max = 0;
    bool ranges = true;
    if (const int rc = frame_sets_check(name, K, Kq, q_frame0, sets, win_lo, win_n, &K_max, &ranges)) return rc;
    constexpr int REFUSED = TF_ATTN_BANK_ONLY | TF_ATTN_SOURCE_ONLY | TF_ATTN_FOLD_SCALE | TF_ATTN_MULTI_V | TF_ATTN_NO_MULTI_V |
                            TF_ATTN_MULTI_V64 | TF_ATTN_RUN_MULTI_V;
    TF_ARG(!(flags & REFUSED), TF_ERR_SHAPE,
           "%s: flags 0x%x -- TF_ATTN_BANK_ONLY / TF_ATTN_SOURCE_ONLY / TF_ATTN_FOLD_SCALE and the multi-edit hints have no "
           "frame-set form", name, flags & REFUSED);
    if (ranges)   // every set a contiguous range: the windowed call (which is the plain call where every range is the bank)
        return tf_ext_attn_fwd_windows(q, k, v, out, K, Kq, q_frame0, S, H, Dh, ld, strides, scale, flags, dtype, win_lo, win_n, ws,
                                       ws_bytes, stream);
    const SetPart fs{sets, K_max};
    return attn_fwd_core(q, k, v, out, K, Kq, q_frame0, S, H, Dh, ld, strides, scale, flags, dtype, ws, ws_bytes, stream, nullptr,
                         nullptr, nullptr, &fs);
}

// Launch plan of tf_ext_attn_fwd_frame_sets for dense tensors (host only): the entry point itself under the plan recorder.
extern "C" int tf_ext_attn_frame_sets_plan(int K, int Kq, int q_frame0, int S, int H, int Dh, int flags, int dtype,
                                           const uint64_t* sets, char* buf, size_t len) {
    TF_ARG(K > 0 && S > 0 && H > 0 && Kq > 0 && Kq <= K, TF_ERR_SHAPE, "tf_ext_attn_frame_sets_plan: K=%d Kq=%d S=%d H=%d", K, Kq,
           S, H);
    void* const ph = reinterpret_cast<void*>((uintptr_t)1 << 12);
    const int64_t ld = (int64_t)H * Dh, fs = (int64_t)S * ld;
    const int64_t strides[9] = {Kq * fs, fs, K * fs, fs, K * fs, fs, Kq * fs, fs, ld};
    TfPlanRec rec{buf, len, 0, 0};
    if (buf && len) buf[0] = 0;
    tf_plan_rec = &rec;
    const int rc = tf_ext_attn_fwd_frame_sets(ph, ph, ph, ph, K, Kq, q_frame0, S, H, Dh, ld, strides, 1.0f, flags, dtype, sets, ph,
                                              tf_ext_attn_workspace_bytes(K, S, H, Dh, dtype), nullptr);
    tf_plan_rec = nullptr;
    if (rc) return rc;
    TF_ARG(rec.used < len, TF_ERR_WORKSPACE, "tf_ext_attn_frame_sets_plan: the plan needs %zu bytes", rec.used + 1);
    return rec.n;
}

// The bank part of a frame-set pass (include/tokenflow_hip.h): tf_ext_attn_fwd_frame_sets with TF_ATTN_BANK_ONLY accepted -- k and
// v hold only the slabs the bank branches read, addressed as in tf_ext_attn_fwd_strided with that flag.  What a frame-sharded rank
// runs over its anchor-extended receive buffer; the source part of a frame-set pass is set-free.  An entry point and its checks:
// attn_fwd_core takes the set table beside the part flags (the multi-edit composition hands it the same pair).
extern "C" int tf_ext_attn_fwd_frame_sets_part(const void* q, const void* k, const void* v, void* out, int K, int Kq, int q_frame0,
                                               int S, int H, int Dh, int64_t ld, const int64_t* strides, float scale, int flags,
                                               int dtype, const uint64_t* sets, void* ws, size_t ws_bytes, void* stream) {
    const char* const name = "tf_ext_attn_fwd_frame_sets_part";
    if (!(flags & TF_ATTN_BANK_ONLY))   // without the flag the call IS tf_ext_attn_fwd_frame_sets (which refuses the source flag)
        return tf_ext_attn_fwd_frame_sets(q, k, v, out, K, Kq, q_frame0, S, H, Dh, ld, strides, scale, flags, dtype, sets, ws,
                                          ws_bytes, stream);
    int win_lo[TF_MAX_WINDOW_FRAMES], win_n[TF_MAX_WINDOW_FRAMES], K_max = 0;
    bool ranges = true;
    if (const int rc = frame_sets_check(name, K, Kq, q_frame0, sets, win_lo, win_n, &K_max, &ranges)) return rc;
    constexpr int REFUSED = TF_ATTN_SOURCE_ONLY | TF_ATTN_FOLD_SCALE | TF_ATTN_MULTI_V | TF_ATTN_NO_MULTI_V | TF_ATTN_MULTI_V64 |
                            TF_ATTN_RUN_MULTI_V;
    TF_ARG(!(flags & REFUSED), TF_ERR_SHAPE,
           "%s: flags 0x%x -- TF_ATTN_SOURCE_ONLY (the source part of a frame-set pass is tf_ext_attn_fwd_strided) / "
           "TF_ATTN_FOLD_SCALE and the multi-edit hints have no frame-set form", name, flags & REFUSED);
    if (ranges)   // every set a contiguous range: the windowed part (the strided call where every range is the bank)
        return tf_ext_attn_fwd_windows_part(q, k, v, out, K, Kq, q_frame0, S, H, Dh, ld, strides, scale, flags, dtype, win_lo, win_n,
                                            ws, ws_bytes, stream);
    const SetPart fs{sets, K_max};
    return attn_fwd_core(q, k, v, out, K, Kq, q_frame0, S, H, Dh, ld, strides, scale, flags, dtype, ws, ws_bytes, stream, nullptr,
                         nullptr, nullptr, &fs);
}

// Launch plan of tf_ext_attn_fwd_frame_sets_part for dense tensors (host only): the entry point itself under the plan recorder.
extern "C" int tf_ext_attn_frame_sets_part_plan(int K, int Kq, int q_frame0, int S, int H, int Dh, int flags, int dtype,
                                                const uint64_t* sets, char* buf, size_t len) {
    TF_ARG(K > 0 && S > 0 && H > 0 && Kq > 0 && Kq <= K, TF_ERR_SHAPE, "tf_ext_attn_frame_sets_part_plan: K=%d Kq=%d S=%d H=%d", K,
           Kq, S, H);
    void* const ph = reinterpret_cast<void*>((uintptr_t)1 << 12);
    const int64_t ld = (int64_t)H * Dh, fs = (int64_t)S * ld;
    const int64_t strides[9] = {Kq * fs, fs, K * fs, fs, K * fs, fs, Kq * fs, fs, ld};
    TfPlanRec rec{buf, len, 0, 0};
    if (buf && len) buf[0] = 0;
    tf_plan_rec = &rec;
    const int rc = tf_ext_attn_fwd_frame_sets_part(ph, ph, ph, ph, K, Kq, q_frame0, S, H, Dh, ld, strides, 1.0f, flags, dtype, sets,
                                                   ph, tf_ext_attn_workspace_bytes(K, S, H, Dh, dtype), nullptr);
    tf_plan_rec = nullptr;
    if (rc) return rc;
    TF_ARG(rec.used < len, TF_ERR_WORKSPACE, "tf_ext_attn_frame_sets_part_plan: the plan needs %zu bytes", rec.used + 1);
    return rec.n;
}

// ---------------------------------------------------------------------------------------------
// Frame-set bank for a multi-edit batch (include/tokenflow_hip.h): the masked composition with the set table handed to every bank
// part -- ONE pre-pass, the injecting edits (pairs in the frame-set four-bank form where it is selected, an odd one in the DUAL set
// launch), the others through their bank-only set launches, then the plain source-only launches.  A table of contiguous ranges is
// handed on as the equivalent window table: the launches of tf_ext_attn_fwd_windows_edits (of tf_ext_attn_fwd_edits_masked where
// every range is the bank).
extern "C" int tf_ext_attn_fwd_frame_sets_edits(const void* q, const void* k, const void* v, void* out, int K, int Kq, int q_frame0,
                                                int S, int H, int Dh, int64_t ld, const int64_t* strides, float scale, int flags,
                                                int dtype, int n_edits, unsigned inject_mask, const uint64_t* sets, void* ws,
                                                size_t ws_bytes, void* stream) {
    const char* const name = "tf_ext_attn_fwd_frame_sets_edits";
    int win_lo[TF_MAX_WINDOW_FRAMES], win_n[TF_MAX_WINDOW_FRAMES], K_max = 0;
    bool ranges = true;
    if (const int rc = frame_sets_check(name, K, Kq, q_frame0, sets, win_lo, win_n, &K_max, &ranges)) return rc;
    // (the multi-edit hints TF_ATTN_MULTI_V / TF_ATTN_NO_MULTI_V / TF_ATTN_MULTI_V64 select the pair form here)
    constexpr int REFUSED = TF_ATTN_BANK_ONLY | TF_ATTN_SOURCE_ONLY | TF_ATTN_FOLD_SCALE | TF_ATTN_RUN_MULTI_V;
    TF_ARG(!(flags & REFUSED), TF_ERR_SHAPE,
           "%s: flags 0x%x -- TF_ATTN_BANK_ONLY / TF_ATTN_SOURCE_ONLY / TF_ATTN_FOLD_SCALE / TF_ATTN_RUN_MULTI_V have no frame-set "
           "form", name, flags & REFUSED);
    if (ranges) {   // the windowed multi-edit call's launches (a checked set table is a valid window table)
        unsigned win[TF_MAX_WINDOW_FRAMES];
        bool full = true;
        for (int i = 0; i < Kq; ++i) {
            win[i] = (unsigned)win_lo[i] | ((unsigned)win_n[i] << 16);
            full = full && win_n[i] == K;
        }
        const WinPart wn{win, K_max};
        return attn_fwd_edits_masked(name, q, k, v, out, K, Kq, q_frame0, S, H, Dh, ld, strides, scale, flags, dtype, n_edits,
                                     inject_mask, ws, ws_bytes, stream, false, 0, full ? nullptr : &wn);
    }
    // (n_edits = 1: the masked composition is attn_fwd_core on today's layout, here with the set table: tf_ext_attn_fwd_frame_sets)
    const SetPart fs{sets, K_max};
    return attn_fwd_edits_masked(name, q, k, v, out, K, Kq, q_frame0, S, H, Dh, ld, strides, scale, flags, dtype, n_edits,
                                 inject_mask, ws, ws_bytes, stream, false, 0, nullptr, &fs);
}

// Launch plan of tf_ext_attn_fwd_frame_sets_edits for dense tensors (host only): the entry point itself under the plan recorder.
extern "C" int tf_ext_attn_frame_sets_edits_plan(int K, int Kq, int q_frame0, int S, int H, int Dh, int n_edits,
                                                 unsigned inject_mask, int flags, int dtype, const uint64_t* sets, char* buf,
                                                 size_t len) {
    TF_ARG(K > 0 && S > 0 && H > 0 && Kq > 0 && Kq <= K, TF_ERR_SHAPE, "tf_ext_attn_frame_sets_edits_plan: K=%d Kq=%d S=%d H=%d", K,
           Kq, S, H);
    void* const ph = reinterpret_cast<void*>((uintptr_t)1 << 12);
    const int64_t ld = (int64_t)H * Dh, fs = (int64_t)S * ld;
    const int64_t strides[9] = {Kq * fs, fs, K * fs, fs, K * fs, fs, Kq * fs, fs, ld};
    TfPlanRec rec{buf, len, 0, 0};
    if (buf && len) buf[0] = 0;
    tf_plan_rec = &rec;
    const int rc = tf_ext_attn_fwd_frame_sets_edits(ph, ph, ph, ph, K, Kq, q_frame0, S, H, Dh, ld, strides, 1.0f, flags, dtype,
                                                    n_edits, inject_mask, sets, ph, (size_t)-1, nullptr);
    tf_plan_rec = nullptr;
    if (rc) return rc;
    TF_ARG(rec.used < len, TF_ERR_WORKSPACE, "tf_ext_attn_frame_sets_edits_plan: the plan needs %zu bytes", rec.used + 1);
    return rec.n;
}

// The bank part of a frame-set multi-edit pass (include/tokenflow_hip.h): tf_ext_attn_fwd_frame_sets_edits with TF_ATTN_BANK_ONLY
// accepted and q / k dense or compact as in tf_ext_attn_fwd_edits_part -- what a frame-sharded rank would run over its
// anchor-extended receive buffer for all E edits at once.  Where every edit's bank part takes the fused small-problem kernel they
// share ONE launch under the one set table (fused[..,sets=E,set]).  A table of contiguous ranges is handed on as the equivalent
// window table (tf_ext_attn_fwd_windows_edits_part; tf_ext_attn_fwd_edits_part where every range is the bank).  The source part of a
// frame-set pass is set-free: tf_ext_attn_fwd_edits_part(TF_ATTN_SOURCE_ONLY).
extern "C" int tf_ext_attn_fwd_frame_sets_edits_part(const void* q, const void* k, const void* v, void* out, int K, int Kq,
                                                     int q_frame0, int S, int H, int Dh, int64_t ld, const int64_t* strides,
                                                     float scale, int flags, int dtype, int n_edits, unsigned inject_mask,
                                                     int qk_compact, const uint64_t* sets, void* ws, size_t ws_bytes,
                                                     void* stream) {
    const char* const name = "tf_ext_attn_fwd_frame_sets_edits_part";
    TF_ARG(qk_compact == 0 || qk_compact == 1, TF_ERR_SHAPE, "%s: qk_compact=%d (0 or 1)", name, qk_compact);
    if (!(flags & TF_ATTN_BANK_ONLY)) {   // without the flag the call IS tf_ext_attn_fwd_frame_sets_edits (which refuses the source flag)
        TF_ARG(!qk_compact || (flags & TF_ATTN_SOURCE_ONLY), TF_ERR_SHAPE,
               "%s: qk_compact=1 without TF_ATTN_BANK_ONLY (the whole call reads dense q / k)", name);
        return tf_ext_attn_fwd_frame_sets_edits(q, k, v, out, K, Kq, q_frame0, S, H, Dh, ld, strides, scale, flags, dtype, n_edits,
                                                inject_mask, sets, ws, ws_bytes, stream);
    }
    int win_lo[TF_MAX_WINDOW_FRAMES], win_n[TF_MAX_WINDOW_FRAMES], K_max = 0;
    bool ranges = true;
    if (const int rc = frame_sets_check(name, K, Kq, q_frame0, sets, win_lo, win_n, &K_max, &ranges)) return rc;
    constexpr int REFUSED = TF_ATTN_SOURCE_ONLY | TF_ATTN_FOLD_SCALE | TF_ATTN_RUN_MULTI_V;
    TF_ARG(!(flags & REFUSED), TF_ERR_SHAPE,
           "%s: flags 0x%x -- TF_ATTN_SOURCE_ONLY (the source part of a frame-set pass is tf_ext_attn_fwd_edits_part) / "
           "TF_ATTN_FOLD_SCALE / TF_ATTN_RUN_MULTI_V have no frame-set form", name, flags & REFUSED);
    if (ranges)   // the windowed part's launches (a checked set table is a valid window table)
        return tf_ext_attn_fwd_windows_edits_part(q, k, v, out, K, Kq, q_frame0, S, H, Dh, ld, strides, scale, flags, dtype, n_edits,
                                                  inject_mask, qk_compact, win_lo, win_n, ws, ws_bytes, stream);
    // (n_edits = 1: the masked composition is attn_fwd_core with the part flag and the set table: tf_ext_attn_fwd_frame_sets_part)
    const SetPart fs{sets, K_max};
    return attn_fwd_edits_masked(name, q, k, v, out, K, Kq, q_frame0, S, H, Dh, ld, strides, scale, flags, dtype, n_edits,
                                 inject_mask, ws, ws_bytes, stream, true, qk_compact, nullptr, &fs);
}

// Launch plan of tf_ext_attn_fwd_frame_sets_edits_part for dense tensors (q / k dense or compact: the plan does not depend on it).
extern "C" int tf_ext_attn_frame_sets_edits_part_plan(int K, int Kq, int q_frame0, int S, int H, int Dh, int n_edits,
                                                      unsigned inject_mask, int qk_compact, int flags, int dtype,
                                                      const uint64_t* sets, char* buf, size_t len) {
    TF_ARG(K > 0 && S > 0 && H > 0 && Kq > 0 && Kq <= K, TF_ERR_SHAPE,
           "tf_ext_attn_frame_sets_edits_part_plan: K=%d Kq=%d S=%d H=%d", K, Kq, S, H);
    void* const ph = reinterpret_cast<void*>((uintptr_t)1 << 12);
    const int64_t ld = (int64_t)H * Dh, fs = (int64_t)S * ld;
    const int64_t strides[9] = {Kq * fs, fs, K * fs, fs, K * fs, fs, Kq * fs, fs, ld};
    TfPlanRec rec{buf, len, 0, 0};
    if (buf && len) buf[0] = 0;
    tf_plan_rec = &rec;
    const int rc = tf_ext_attn_fwd_frame_sets_edits_part(ph, ph, ph, ph, K, Kq, q_frame0, S, H, Dh, ld, strides, 1.0f, flags, dtype,
                                                         n_edits, inject_mask, qk_compact, sets, ph, (size_t)-1, nullptr);
    tf_plan_rec = nullptr;
    if (rc) return rc;
    TF_ARG(rec.used < len, TF_ERR_WORKSPACE, "tf_ext_attn_frame_sets_edits_part_plan: the plan needs %zu bytes", rec.used + 1);
    return rec.n;
}
