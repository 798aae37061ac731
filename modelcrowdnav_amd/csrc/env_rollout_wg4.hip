// env_rollout_wg4.hip -- the four-wavefront form of the fused T-step rollout (env_rollout_quad.hip has the other two and the
// dispatch): 8 envs x 5 humans per workgroup, three float32 ORCA wavefronts and one float64 wavefront.  A translation unit
// of its own because it is built WITHOUT the SLP vectoriser (Makefile): the packed float32 instructions the vectoriser
// forms in the ORCA solve cost a wavefront that shares its SIMD 8.75 cycles each, plus the moves that pair their operands,
// and the scalar instructions they stand for 4.6 - 5.0 (profiles/r04_valu_issue.txt, profiles/r18_orca_issue.txt).  The
// other forms keep the flags, and so the code, they had.
#include "env_rollout_common.hpp"
#include "wg4_barrier_plan.hpp"

namespace mcn {

// Four-wavefront form (env_rollout_wg4_kernel): workgroups of EW envs on FOUR wavefronts -- three ORCA wavefronts
// for the EW * NT quads, dealt BY ENV: ORCA wavefront w holds envs 3 w .. 3 w + 2 of the workgroup (wavefront 2 two envs,
// 10 quads), quad 5 le + h of the wavefront is (env 3 w + le, human h), so no env straddles two wavefronts and a quad's
// four candidates sit in its own wavefront; and one float64 wavefront with eight
// lanes per env: lane 8 g + h is (env g, human h) for h < NT, lanes h >= NT are idle (they hold no distance: +inf, and
// no overlap), so an env's minimum distance and overlap count are three DPP exchanges inside its eight lanes.
// The float64 wavefront is workgroup wave 3: the hardware deals a workgroup's waves one to each SIMD and starts the
// two workgroups of a CU on different SIMDs, so their float64 wavefronts do not share one (census in
// profiles/r13_rollout_roles.txt).
// The two-wavefront form gives every 3 envs a float64 wavefront of their own, which repeats each swept-circle test on 4
// lanes and the ladder on 20; here 8 envs share it, and 4096 envs x 5 humans become 512 workgroups = exactly two
// wavefronts on each of the chip's 1024 SIMDs instead of two on some and three on others.
//
// The float64 wavefront OWNS every float64 value of the env: the robot, the clock, the records and the humans' position,
// velocity, goal, radius, v_pref and human_times -- one human per lane, loaded in its prologue, integrated or restarted
// from the pool by it, stored in its epilogue.  The ORCA wavefronts run quad_orca_core (quad_common.hpp) and publish the
// new velocity as two floats.  Each quad also carries a float64 COPY of its human's position and goal (8 VGPRs of the
// ~59 the ORCA role leaves unused in the kernel's allocation, which is the float64 role's): after the solve every lane of
// the quad executes the owner's statements on it, pos + (double)r * dt and quad_orca_position_pack(pos, goal) -- the
// same operations on the same operands, so the same bits as the owner's -- and has its next step's position operands
// without waiting for anybody.  A candidate's position and velocity come from a quad of the same wavefront, through a
// slot of the wavefront's own line table, which is dead between two solves.  So a normal step has ONE workgroup barrier,
// the hand-off: before it the ORCA wavefronts publish (rx, ry) to s_res[t & 1] and the float64 wavefront the workgroup's
// restart flag to s_flag[t & 1]; behind it the ORCA wavefronts read the flag and their candidate's slot (one LDS round trip)
// and start the next solve, and the float64 wavefront reads s_res[t & 1], integrates its own copy and goes on with its
// step: s_hpos, velocity register, human_times, then the next step's swept test, pairs, ladder, accounting and restart
// fetch.  Both arrays are indexed by step parity: what is read behind the hand-off of step t is next written before the
// hand-off of step t + 2, i.e. behind that of step t + 1, which the reader reaches only with its reads complete.
//
// What stays off the ORCA wavefronts' step:
//   * the velocity never leaves float32: the solve's velocity operands are the floats the ORCA wavefronts produced
//     (float32 -> float64 -> float32 gives the same bits back): the owner's are the (rx, ry) its quad still holds, the
//     candidate's come with its position;
//   * frad and the maximum speed change only on a restart and live in s_inv, written in the prologue and by restart lanes;
//     the ORCA wavefronts keep them, and the candidate's frad, in registers from one restart step to the next;
//   * what a restarted human publishes (start velocity, s_inv) is converted BEFORE the hand-off, where the
//     float64 wavefront would idle anyway;
//   * the 2-D LP's four take steps decide from min(fail, code_i), known before the step's test (QuadTable::lean_take,
//     quad_take_plan.hpp): five instructions in a row per step for eight, ten fewer in the loop.  On the SIMDs that hold
//     two ORCA wavefronts an instruction costs its issue slot on or off the chain (profiles/r30_rollout_parallel_takes.txt:
//     the form that evaluated all sixteen tests at once had a shorter chain, thirty instructions more, and lost 4 %).
//     The 3-D LP candidate's three take steps are the same lean steps (QuadTable::lean_lp3);
//   * the rank's four quad broadcasts of the key are folded into the subtractions that read them (QuadTable::fold_rank:
//     four v_sub_u32_dpp).  The take steps' candidate broadcasts folded into v_cndmask_b32_dpp need inline asm, which the
//     compiler cannot schedule around: eight instructions fewer, 0.8 % slower (profiles/r31_rollout_dpp_fold.txt);
//   * the three range guards of a normal step (half-plane, clip, 1-D LP discriminant) compute the fast values first and
//     replace them under a branch marked unlikely (QuadTable::straight; fast_f32.hpp: FAST_FIRST): each guard is one
//     not-taken s_cbranch_scc0 where the step went to a block behind the loop's end and back, 98 cycles a round trip for a
//     wavefront alone on its SIMD (profiles/r32_branch_cost.txt), +2.2 % (profiles/r32_rollout_branch_layout.txt).  The one
//     taken branch left before the hand-off is the skip over the 3-D LP: moving that loop out of line measured nothing.
// Each value is produced by the operation, on the operands, that the other forms use, so the same bits.
//
// RESTART STEPS (some env of the workgroup ends: roughly one workgroup-step in ten) and the launch's first solve take the
// SLOW PATH.  The float64 wavefront knows the done flags when its ladder ends and stores the workgroup's there: word EW of
// s_flag[t & 1].  Behind the hand-off of such a step it stores each env's flag (words 0 .. EW - 1) and its restart lanes
// stage the new human -- float64 position and goal in two slots of the human's ORCA wavefront's line table (dead in that
// window as well; other slots than the candidate exchange uses), the start velocity over the solve's in s_res[t & 1],
// (frad, maximum speed) in s_inv -- and all four wavefronts meet at a second barrier, `staged`, behind which the ORCA
// wavefronts read every operand from LDS: velocities, s_inv, and for the quads of a restarted env (its flag word) position
// and goal of their human and the position of their candidate; the others keep their copy.  The prologue stages every
// human the same way, with every flag set, as "step -1" (parity 1), and its barrier, `seed`, stands for both.  No third
// barrier fences these reads from the next publish as it did while s_res was one buffer: the next publish goes to the
// other parity.  Which barriers a role executes when is wg4_step_barriers (wg4_barrier_plan.hpp), one function for both
// loops: all four wavefronts execute the same barriers in the same order on every path, the last step's included.
// Step t and who touches what (W = writes, R = reads; f64 = the float64 wavefront; p = t & 1):
//   A  the barrier before (hand-off or staged of step t - 1, or the seed) -> hand-off of step t
//   B  hand-off of step t -> the next barrier (a normal step: this is the head of step t + 1's A; a restart step: staged)
//   C  restart steps only: staged -> hand-off of step t + 1 (the head of step t + 1's A)
//                  A                                  B                                          C
//   s_res[p]       W ORCA (end of the solve)          R f64 (own slot); then W f64 restart lanes  R ORCA (own, candidate)
//   s_inv          --                                 W f64 restart lanes                         R ORCA (own, candidate)
//   s_flag[p]      W f64 word EW (behind its ladder)  R ORCA word EW; W f64 words 0 .. EW - 1     R ORCA (its env's word)
//   s_lines        W/R its ORCA wavefront: the solve, R its ORCA wavefront (exchange slots);      R its ORCA wavefront
//                  then W the exchange slots          W f64 restart lanes (staging slots)         (staging slots)
//   s_hpos/s_hrad  R f64 (pairs)                      W f64 behind its last barrier of the step: its own arrays
// The slot an ORCA wavefront reads in B is its own wavefront's write of A; the hand-off's fences order them.  A restarted
// env's quads integrate the old human before the hand-off and exchange its position behind it; the slow path overwrites
// all of that.
//
// The float64 wavefront's ladder, Explorer accounting, finished-episode stores, robot integrate / restart and the epilogue
// are the TWIN of env_rollout_quad_kernel's (env_rollout_quad.hip): a change to either is made to both.  The text is
// not shared: with the tail in common functions this kernel's two forms came out at 1791 and 2811 instructions for
// 1804 and 2840 with another SGPR use, and the older kernel lost registers to scratch (profiles/r19_env_refactor.txt,
// section 4), on the path the benchmark's headline runs.  The humans' integrate / restart holds the twin's statements
// (pos + (double)r * dt, the pool fetch, human_times) in another order: the restart fetch before the hand-off, the
// integrate behind it, then the velocity register and human_times; and the integrate and the position pack are
// executed a second time, on the ORCA quads' copy.
template <int NT>
struct Wg4 {
    static_assert(NT == 5, "the four-wavefront form is built for 5 humans only");
    static constexpr int EW = 8;                              // envs per workgroup
    static constexpr int NQ = EW * NT;                        // populated quads = populated float64 lanes: 40 of 48 / 64
    static constexpr int EPW = 3;                             // envs per ORCA wavefront: 3 + 3 + 2, 15 / 15 / 10 of 16 quads
    static_assert(EPW * NT <= 16 && 3 * EPW >= EW, "an env's quads share a wavefront and three wavefronts hold them all");
    // A wavefront's line table (64 float4 slots) between two solves: slot q = quad q's (px, py, rx, ry) for the quads
    // whose candidate it is; slots STAGE + 2 q, + 1 = the float64 position and goal a restart lane stages for quad q
    static constexpr int STAGE = 16;
    static_assert(STAGE + 2 * 16 <= 64, "the staging slots lie inside the wavefront's table");
    static constexpr int FLAGS = 16;                          // words per parity of s_flag: EW env flags, then the workgroup's
    static_assert(EW < FLAGS, "one word per env and one for the workgroup");
};

// value of the lane a DPP control selects (all lanes of the wavefront active)
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) { return __builtin_amdgcn_mov_dpp(v, CTRL, 0xf, 0xf, true); }
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v)
{
    const long long b = __builtin_bit_cast(long long, v);
    const int lo = dpp_i<CTRL>((int)b), hi = dpp_i<CTRL>((int)(b >> 32));
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}
constexpr int DPP_QUAD_XOR1 = 0xB1, DPP_QUAD_XOR2 = 0x4E, DPP_ROW_HALF_MIRROR = 0x141;   // quad_perm [1,0,3,2], [2,3,0,1]

// a double2 as the float4 of the same 16 bytes and back: whole-register moves, for the slots of a line table
__device__ __forceinline__ float4 d2_as_f4(double2 v)
{
    const long long x = __builtin_bit_cast(long long, v.x), y = __builtin_bit_cast(long long, v.y);
    return make_float4(__builtin_bit_cast(float, (int)x), __builtin_bit_cast(float, (int)(x >> 32)),
                       __builtin_bit_cast(float, (int)y), __builtin_bit_cast(float, (int)(y >> 32)));
}
__device__ __forceinline__ double2 f4_as_d2(float4 v)
{
    const long long x = ((long long)__builtin_bit_cast(int, v.y) << 32) | (unsigned int)__builtin_bit_cast(int, v.x);
    const long long y = ((long long)__builtin_bit_cast(int, v.w) << 32) | (unsigned int)__builtin_bit_cast(int, v.z);
    return make_double2(__builtin_bit_cast(double, x), __builtin_bit_cast(double, y));
}

// the staging slots of the human in hand-off slot `hs` = env * NT + human, in the table of the ORCA wavefront that holds it
template <int NT>
__device__ __forceinline__ float4 *wg4_stage(float4 *lines, int hs)
{
    constexpr int PER = Wg4<NT>::EPW * NT;                      // hand-off slots per ORCA wavefront, in order
    const int w = hs / PER;
    return lines + w * 64 + Wg4<NT>::STAGE + 2 * (hs - w * PER);
}

// `n` workgroup barriers, n from wg4_step_barriers with the flags the caller knows at that point spelt as constants, so that
// the loop folds (with a run-time count the compiler keeps a counted loop round the s_barrier)
__device__ __forceinline__ void wg4_sync(int n)
{
    for (int i = 0; i < n; ++i) __syncthreads();
}

template <int NT, int VIS, bool UNI>
__device__ __forceinline__ void rollout_wg4(const StepParams &p, const int T)
{
    static_assert(VIS == 0, "the four-wavefront form is built for an invisible robot only");
    constexpr int EW = Wg4<NT>::EW, NQ = Wg4<NT>::NQ, EPW = Wg4<NT>::EPW, STAGE = Wg4<NT>::STAGE, FLAGS = Wg4<NT>::FLAGS;
    // hand-off arrays, one slot per (env, human), slot = env * NT + human.  s_res: the human's new velocity, two buffers
    // by step parity, written by the ORCA wavefronts at the end of a solve (and by restart lanes: the start velocity),
    // read by the float64 wavefront every step and by the slow path.  s_inv = (frad, maximum speed), written in the
    // prologue and by restart lanes, read by the slow path.  s_hpos / s_hrad, the float64 position and radius the overlap
    // pairs read from partner lanes, are the float64 wavefront's own.
    __shared__ float2 s_res[2 * NQ], s_inv[NQ];
    // per parity: words 0 .. EW - 1, env g restarts on this step; word EW, some env of the workgroup does.  The other
    // words are room earlier layouts used: the workgroup's LDS, and with it the CU's, stays what it was
    __shared__ int s_flag[4 * NQ];
    static_assert(2 * FLAGS <= 4 * NQ, "two parities of flags");
    __shared__ double2 s_hpos[NQ];
    __shared__ double s_hrad[NQ];
    // the ORCA wavefronts' sorted half-planes (quad_common.hpp: QuadTable): 64 slots each, private to the wavefront.  A lane
    // reads its quad's four slots, its own, and the two operands of its pass-A intersection (lp1_spread): seven reads.
    // Between two solves: the candidate exchange and the restart staging (Wg4)
    __shared__ float4 s_lines[3 * 64];
    STAMP(0);
    STAMP_WHERE();
#ifdef MCN_DIAG
    if (p.debug_noop) return;
#endif
    const int tid = threadIdx.x;
    // wave-uniform by construction, and known to be: each role runs its own step loop, barriers included
    const int role = __builtin_amdgcn_readfirstlane(tid >> 6);      // 0-2: ORCA, 3: float64 state, ladder, records
    const unsigned chunk_ = xcd_chunk();
    const mcn_env_cfg &c = p.cfg;
    const mcn_rollout &ro = p.roll;

    if (role < 3) {
        // ---------------- ORCA wavefronts: the float32 solve and the integrate of their copy ----------------
        const int lane = tid & 63, k = tid & 3, q = lane >> 2;  // quad q of this wavefront
        const int le = q / NT, h = q - le * NT;                  // (env of the wavefront, human)
        const int ge = role * EPW + le;                          // env of the workgroup
        const bool pop = le < EPW && ge < EW;                    // idle quads (and envs >= E) hold no half-plane, write nothing
        const bool active = pop && (long)chunk_ * EW + ge < p.E;
        const int hi = pop ? ge * NT + h : 0;                    // hand-off slot of this quad's human (idle quads read slot 0)
        const bool cand_h = k < NT - 1;                          // candidate is another human
        const int j = cand_h ? k + (k >= h ? 1 : 0) : h;
        const int ci = pop ? ge * NT + j : 0;                    // the candidate's hand-off slot ...
        const int cq = pop ? le * NT + j : 0;                    // ... and its quad in this wavefront
        const int fi = pop ? ge : 0;                             // the env's flag word
        const bool publish = pop && k == 0;
        const float inv_th = in_vgpr(1.0f / c.orca_time_horizon), inv_ts = in_vgpr(1.0f / (float)c.time_step);
        const double dt = in_vgpr(c.time_step);
        float4 *const tab = s_lines + role * 64;
        const float4 *const stage = tab + STAGE + 2 * (pop ? q : 0), *const cstage = tab + STAGE + 2 * cq;
        // what a normal step keeps in registers: the float64 copy of position and goal, the position operands formed from
        // it, own velocity v, the candidate's position and velocity, (frad, ms) and the candidate's frad
        double2 pos = make_double2(0, 0), goal = make_double2(0, 0);
        float4 P = make_float4(0, 0, 0, 0);
        float vx = 0, vy = 0, cpx = 0, cpy = 0, cvx = 0, cvy = 0, frad = 0, ms = 0, orad = 0;
        // Slow path, behind a seed or staged barrier: every operand from LDS, one round trip for the nine reads (the empty
        // asm needs them all).  `par`: parity of the step whose hand-off came before (the prologue's: 1).  The velocities
        // are what the solves or the prologue left with the restart lanes' overwritten, frad / ms as the restart lanes
        // left them; position and goal are staged for restarted envs only, the other quads keep theirs.
        auto reload = [&](const int par) {
            const float2 *res = s_res + par * NQ;
            float2 v = res[hi], cv = res[ci];
            float2 fm = s_inv[hi];
            float od = s_inv[ci].x;                              // the candidate's own frad
            int mine = s_flag[par * FLAGS + fi];
            float4 sp = stage[0], sg = stage[1], sc = cstage[0];
            asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(cv.x), "+v"(cv.y), "+v"(fm.x), "+v"(fm.y), "+v"(od), "+v"(mine));
            asm volatile("" : "+v"(sp.x), "+v"(sp.y), "+v"(sp.z), "+v"(sp.w), "+v"(sg.x), "+v"(sg.y), "+v"(sg.z), "+v"(sg.w),
                              "+v"(sc.x), "+v"(sc.y), "+v"(sc.z), "+v"(sc.w));
            vx = v.x; vy = v.y; cvx = cv.x; cvy = cv.y; frad = fm.x; ms = fm.y; orad = od;
            if (mine != 0) {
                pos = f4_as_d2(sp);
                goal = f4_as_d2(sg);
                const double2 cpos = f4_as_d2(sc);
                P = quad_orca_position_pack(pos, goal);
                cpx = (float)cpos.x; cpy = (float)cpos.y;        // the candidate's own (float)pos
            }
        };
        wg4_sync(wg4_step_barriers(kWg4Orca, true, false, false).seed);      // the float64 wavefront has staged every human
        reload(1);
        STAMP(1);

        for (int t = 0; t < T; ++t) {
            float rx, ry;
            quad_orca_core(c, lane, k, cand_h && active, make_float4(P.x, P.y, vx, vy), make_float4(P.z, P.w, frad, ms),
                           make_float4(cpx, cpy, cvx, cvy), orad, inv_th, inv_ts, rx, ry, QuadTable{tab});
            // the owner's integrate on this quad's copy, and the next step's position operands from it
            pos = make_double2(pos.x + (double)rx * dt, pos.y + (double)ry * dt);
            P = quad_orca_position_pack(pos, goal);
            const int par = t & 1;
            if (publish) {
                s_res[par * NQ + hi] = make_float2(rx, ry);
                tab[q] = make_float4(P.x, P.y, rx, ry);          // for the quads whose candidate this human is
            }
            if (t < 20) STAMP(40 + t);
            const Wg4StepBarriers normal = wg4_step_barriers(kWg4Orca, false, false, t + 1 == T);
            wg4_sync(normal.handoff);                            // the hand-off: the humans' new velocities, the flags
            // the workgroup's restart flag and the candidate's slot, one LDS round trip (the hand-off's fences order the
            // slot's read behind every quad's write); the own new velocity is (rx, ry), identical on the quad's lanes
            int flag = s_flag[par * FLAGS + EW];
            float4 x = tab[cq];
            asm volatile("" : "+v"(flag), "+v"(x.x), "+v"(x.y), "+v"(x.z), "+v"(x.w));
            const bool slow = __builtin_amdgcn_readfirstlane(flag) != 0;
            vx = rx; vy = ry; cpx = x.x; cpy = x.y; cvx = x.z; cvy = x.w;
            const Wg4StepBarriers plan = wg4_step_barriers(kWg4Orca, false, slow, t + 1 == T);
            if (plan.staged) {
                wg4_sync(wg4_step_barriers(kWg4Orca, false, true, t + 1 == T).staged);      // the new humans are staged
                reload(par);
            }
            if (t < 37) STAMP(2 + t);
        }
    } else {
        // ---------------- float64 wavefront: lane 8 g + h = (env g, human h), h >= NT idle ----------------
        static_assert(EW * 8 == 64, "eight lanes per env fill the wavefront");
        const double dt = in_vgpr(c.time_step);
        const bool do_reset = p.has_roll && ro.pool_hpos != nullptr;
        const int l = tid & 63;
        const int g = l >> 3, h = l & 7;
        const bool pop = h < NT;
        const int hs = g * NT + (pop ? h : 0);                   // LDS slot of (env g, human h); idle lanes alias human 0
        const long e = (long)chunk_ * EW + g;
        const bool active = pop && e < p.E;
        const long eb = e < p.E ? e : 0;                         // idle lanes carry the env's robot too: nothing is stored
        const long a = eb * NT + (pop ? h : 0);                  // ... and a human (envs >= E: env 0's), read-only
        const bool lead = active && h == 0;                      // owns the per-env records
        constexpr bool unicycle = UNI;
        const bool has_state = p.has_roll && ro.state != nullptr;
        const bool track = c.track_human_times && p.st.human_times != nullptr;

        // the humans' float64 state lives here, one human per lane
        double2 pos = reinterpret_cast<const double2 *>(p.st.hpos)[a];
        double2 vel = reinterpret_cast<const double2 *>(p.st.hvel)[a];
        double2 goal = reinterpret_cast<const double2 *>(p.st.hgoal)[a];
        double rad = p.st.hrad[a];
        double vpref = p.st.hvpref[a];
        double htime = p.st.human_times ? p.st.human_times[a] : 0.0;
        double hax = 0, hay = 0;
        double2 rpos = reinterpret_cast<const double2 *>(p.st.rpos)[eb];
        double2 rvel = reinterpret_cast<const double2 *>(p.st.rvel)[eb];
        double2 rgoal = reinterpret_cast<const double2 *>(p.st.rgoal)[eb];
        const double rrad = p.st.rrad[eb];
        double gtime = p.st.gtime[eb];
        double rtheta = p.st.rtheta ? p.st.rtheta[eb] : 0.0;
        // the robot, the clock and the Explorer record are held redundantly by the env's eight lanes
        mcn_roll_rec rs = {0, 0, 0, 0, 0, 0};
        if (has_state) rs = ro.state[eb];
        const double2 *act_ptr = reinterpret_cast<const double2 *>(p.actions) + eb;
        const long act_stride = in_vgpr((long)p.E);
        const double *disc_table = in_vgpr(ro.disc_table);
        const int disc_last = in_vgpr(ro.disc_len - 1);
        const bool has_theta = p.st.rtheta != nullptr;
        double2 act_next = *act_ptr;
        double o_rew = 0, o_dmin = 0;
        int o_dn = 0, o_inf = 0, o_hh = 0;
        // the ladder's constants stay in vector registers (the humans' state took the room the rare time limit and the
        // restart stride had there: those are a kernel-argument read and scalars again)
        const double k_timeout_at = in_vgpr(c.time_limit - 1);
        const double k_collision = in_vgpr(c.collision_penalty), k_success = in_vgpr(c.success_reward);
        const double k_discomfort = in_vgpr(c.discomfort_dist), k_factor = in_vgpr(c.discomfort_penalty_factor);
        const int k_stride = ro.case_stride, k_pool = ro.pool_size;
        const bool count_hh = c.count_hh != 0;
        // the first solve's operands: the loaded state is staged as a restart stages a new human, every flag set, in the
        // buffers of parity 1 ("step -1")
        {
            float4 A, B;
            quad_orca_operands(c, pos, vel, goal, rad, vpref, A, B);
            if (pop) {
                float4 *const stage = wg4_stage<NT>(s_lines, hs);
                stage[0] = d2_as_f4(pos); stage[1] = d2_as_f4(goal);
                s_res[NQ + hs] = make_float2(A.z, A.w);
                s_inv[hs] = make_float2(B.z, B.w);
                s_hpos[hs] = pos; s_hrad[hs] = rad;
            }
            s_flag[FLAGS + g] = 1;
            s_flag[FLAGS + EW] = 1;
        }
        wg4_sync(wg4_step_barriers(kWg4Float64, true, false, false).seed);
        STAMP(1);

        for (int t = 0; t < T; ++t) {
            const double2 act = act_next;
            act_ptr += act_stride;
            if (t + 1 < T) act_next = *act_ptr;
            double ep_disc = 0;
            if (has_state) ep_disc = disc_table[rs.ep_steps < disc_last ? rs.ep_steps : disc_last];

            // ---- K2: the swept circle of human h; the env's unordered human pairs spread over its lanes ----
            double2 eff = act;
            if (unicycle) {
                eff.x = act.x * cos(act.y + rtheta);
                eff.y = act.x * sin(act.y + rtheta);
            }
            double cd;
            {
                const double px = pos.x - rpos.x, py = pos.y - rpos.y;
                const double vx = vel.x - eff.x, vy = vel.y - eff.y;
                cd = p2s_origin(px, py, px + vx * dt, py + vy * dt) - rad - rrad;
            }
            cd = pop ? cd : INFINITY;
            // Lane h takes the pairs (h, h + d mod NT) for d = 1 .. NT / 2: NT is odd, so that is every unordered pair
            // exactly once.  The two-wavefront form tests a pair on the quad of its LOWER
            // human a against candidate b > a: sqrt(s2) - rad_a - rad_b, so the radii are put in that order here; s2 itself
            // does not see the order (the differences only change sign).  Same conservative screen for the sqrt.
            // Both pairs go behind ONE screen: the exact tests are the same, taken only when some lane of the
            // wavefront is within reach in either pair.
            int hh = 0;
            {
                static_assert(NT / 2 == 2, "two pairs per lane");
                double s2[2], ra[2], rb[2];
                bool near_any = false;
                const bool counted = active & count_hh;
#pragma unroll
                for (int d = 1; d <= NT / 2; ++d) {
                    const int jj = h + d >= NT ? h + d - NT : h + d;
                    const int pi = g * NT + (pop ? jj : 0);
                    const double2 ppos = s_hpos[pi];
                    const double prad = s_hrad[pi];
                    ra[d - 1] = jj > h ? rad : prad; rb[d - 1] = jj > h ? prad : rad;
                    const double dx = pos.x - ppos.x, dy = pos.y - ppos.y;
                    s2[d - 1] = dx * dx + dy * dy;
                    const double reach = ra[d - 1] + rb[d - 1] + 1e-6;
                    near_any |= counted & (s2[d - 1] < reach * reach);
                }
                if (__any(near_any)) {
                    DIAG_COUNT(2);
#pragma unroll
                    for (int d = 0; d < NT / 2; ++d)
                        hh += (counted & ((sqrt(s2[d]) - ra[d] - rb[d]) < 0)) ? 1 : 0;
                }
            }
            // the env's minimum and overlap count, on all eight of its lanes: min over numbers does not see the order
            // (no operand is -0: a difference of equal values is +0; a NaN loses to any number, and the idle lanes'
            // +inf keeps an all-NaN env at +inf, which is what min(+inf, NaN, ...) gave in lane order)
            double dmin = cd;
            int hh_sum = hh;
            dmin = fmin(dmin, dpp_d<DPP_QUAD_XOR1>(dmin));       hh_sum += dpp_i<DPP_QUAD_XOR1>(hh_sum);
            dmin = fmin(dmin, dpp_d<DPP_QUAD_XOR2>(dmin));       hh_sum += dpp_i<DPP_QUAD_XOR2>(hh_sum);
            dmin = fmin(dmin, dpp_d<DPP_ROW_HALF_MIRROR>(dmin)); hh_sum += dpp_i<DPP_ROW_HALF_MIRROR>(hh_sum);

            // ---- K3: ladder, on every lane of the env ----
            double endx, endy, new_theta = rtheta, nrvx, nrvy;
            if (unicycle) {
                const double th = rtheta + act.y;
                endx = rpos.x + cos(th) * act.x * dt;
                endy = rpos.y + sin(th) * act.x * dt;
                new_theta = pymod(rtheta + act.y, 2 * M_PI);
                nrvx = act.x * cos(new_theta); nrvy = act.x * sin(new_theta);
            } else {
                endx = rpos.x + act.x * dt; endy = rpos.y + act.y * dt;
                nrvx = act.x; nrvy = act.y;
            }
            bool reaching = false;
            {
                const double gx = endx - rgoal.x, gy = endy - rgoal.y, near = rrad + 1e-6;
                if (__any(gx * gx + gy * gy < near * near)) DIAG_COUNT(3);
                if (__any(gx * gx + gy * gy < near * near)) reaching = norm2(gx, gy) < rrad;
            }
            double rew; int inf, dn;
            if (gtime >= k_timeout_at)          { rew = 0; dn = 1; inf = MCN_INFO_TIMEOUT; }
            else if (dmin < 0)                  { rew = k_collision; dn = 1; inf = MCN_INFO_COLLISION; }
            else if (reaching)                  { rew = k_success; dn = 1; inf = MCN_INFO_REACHGOAL; }
            else if (dmin < k_discomfort)       { rew = (dmin - k_discomfort) * k_factor * dt; dn = 0; inf = MCN_INFO_DANGER; }
            else                                { rew = 0; dn = 0; inf = MCN_INFO_NOTHING; }
            o_rew = rew; o_dmin = dmin; o_dn = dn; o_inf = inf; o_hh = hh_sum;
            const double t_new = gtime + dt;
            // the workgroup's restart flag as soon as the done flags are known: the store is long complete when this
            // wavefront reaches the hand-off (issued there, the barrier's wait for it sat on the chain of every step on
            // which this wavefront is the last to arrive: the unicycle robot's)
            const bool restart = do_reset && dn;
            const bool any_restart = __any(restart);             // roughly one workgroup-step in ten
            const int par = t & 1;
            s_flag[par * FLAGS + EW] = any_restart ? 1 : 0;      // (every lane the same word: no exec mask to set up)

            // ---- Explorer accounting: every lane of the env updates its copy; the stores are the lead lane's ----
            const int case_g = rs.next_case;
            if (has_state) {
                bool danger = inf == MCN_INFO_DANGER;
                if (danger) {
                    const KernargPtr kp = kernarg_here();
                    const int lim = kp->roll.danger_episodes, sf = kp->roll.danger_short_from;
                    danger = lim <= 0 || rs.fin_count < lim - ((sf > 0 && e >= sf - 1) ? 1 : 0);
                }
                rs.danger_count += danger ? 1 : 0;
                rs.danger_dist_sum = danger ? rs.danger_dist_sum + dmin : rs.danger_dist_sum;
                const double ret = rs.ep_return + ep_disc * rew;
                if (lead && dn) {
                    const int kf = rs.fin_count;
                    const KernargPtr kp = kernarg_here();
                    const int fin_slots = kp->roll.fin_slots;
                    double *fin_return = kp->roll.fin_return, *fin_time = kp->roll.fin_time;
                    uint8_t *fin_info = kp->roll.fin_info;
                    const bool keep = (fin_slots == 1) || (kf < fin_slots);
                    const long rec = (long)(fin_slots == 1 ? 0 : kf) * kp->E + e;
                    if (keep && fin_return) fin_return[rec] = ret;
                    if (keep && fin_time)   fin_time[rec] = (inf == MCN_INFO_TIMEOUT) ? kp->cfg.time_limit : t_new;
                    if (keep && fin_info)   fin_info[rec] = (uint8_t)inf;
                }
                rs.fin_count += dn;
                rs.ep_return = dn ? 0.0 : ret;
                rs.ep_steps = dn ? 0 : rs.ep_steps + 1;
                if (do_reset) {
                    int nc = rs.next_case + k_stride;
                    nc = nc >= k_pool ? nc - k_pool : nc;
                    rs.next_case = dn ? nc : rs.next_case;
                }
            }

            // ---- robot: integrate, or back to the start pose ----
            if (do_reset && dn) {
                const KernargPtr kp = kernarg_here();
                const double k_theta0 = kp->roll.robot_theta0;
                rpos = make_double2(kp->roll.robot_start[0], kp->roll.robot_start[1]);
                rgoal = make_double2(kp->roll.robot_goal[0], kp->roll.robot_goal[1]);
                rvel = make_double2(0, 0);
                if (has_theta) rtheta = k_theta0;
                gtime = 0;
            } else {
                rpos = make_double2(endx, endy);
                rvel = make_double2(nrvx, nrvy);
                if (unicycle) rtheta = new_theta;
                gtime = t_new;
            }

            // ---- humans of a finished env restart from the scenario pool NOW, while this wavefront would wait at the hand-off
            //      for the ORCA ones anyway (it knows the done flag first): the case is fetched straight into the state
            //      registers (nothing below reads the old one: the swept circle, the pairs and the ladder are done) and
            //      converted; behind the hand-off a restart lane only stores what it holds here ----
            float2 n_fvel = make_float2(0, 0), n_inv = make_float2(0, 0);
            if (restart) {
                DIAG_COUNT(1);
                if (active) {                                    // (idle lanes keep what they had)
                    const long pa = (long)case_g * NT + h;
                    const KernargPtr kp = kernarg_here();
                    const double2 *pool_hvel = reinterpret_cast<const double2 *>(kp->roll.pool_hvel);
                    vel = make_double2(0, 0);                    // (before the loads: nothing here waits for one)
                    if (pool_hvel) vel = pool_hvel[pa];
                    pos = reinterpret_cast<const double2 *>(kp->roll.pool_hpos)[pa];
                    goal = reinterpret_cast<const double2 *>(kp->roll.pool_hgoal)[pa];
                    rad = kp->roll.pool_hrad[pa];
                    vpref = kp->roll.pool_hvpref[pa];
                }
                htime = 0;
                // every float converted from the new float64 state, as the prologue does for a loaded one (position and
                // goal go to the ORCA quads as float64: they form the position operands themselves)
                float4 A, B;
                quad_orca_operands(c, pos, vel, goal, rad, vpref, A, B);
                // (pinned: not to be sunk behind the barrier)
                n_fvel = make_float2(in_vgpr(A.z), in_vgpr(A.w));
                n_inv = make_float2(in_vgpr(B.z), in_vgpr(B.w));
            }

            if (t < 20) STAMP(40 + t);
            const Wg4StepBarriers plan = wg4_step_barriers(kWg4Float64, false, any_restart, t + 1 == T);
            wg4_sync(plan.handoff);                              // the hand-off: the humans' new velocities
            {
                const float2 r = s_res[par * NQ + hs];
                hax = (double)r.x; hay = (double)r.y;            // (restart lanes too: the epilogue's human_act)
            }
            if (plan.staged) {
                // restart steps only: the new humans for the ORCA quads, who re-read every operand behind the barrier
                // (stores under their own mask; a restart lane's read of s_res above precedes its write in program order)
                // Every address of this rare block is formed here, from the one index the step keeps (opaque, so that
                // nothing of it is hoisted into registers the loop would hold): the env's flag word, read by the slow
                // path only, and the staging slots.
                int hs2 = hs;
                asm volatile("" : "+v"(hs2));
                s_flag[par * FLAGS + hs2 / NT] = restart ? 1 : 0;   // (an env's eight lanes the same word)
                if (pop && restart) {
                    float4 *const stage = wg4_stage<NT>(s_lines, hs2);
                    stage[0] = d2_as_f4(pos); stage[1] = d2_as_f4(goal);
                    s_res[par * NQ + hs2] = n_fvel; s_inv[hs2] = n_inv;
                }
                wg4_sync(wg4_step_barriers(kWg4Float64, false, true, t + 1 == T).staged);
            }
            if (t < 37) STAMP(2 + t);

            // ---- this wavefront's own copy and arrays, the velocity register, the clock of the step just taken ----
            if (!restart) {
                pos = make_double2(pos.x + hax * dt, pos.y + hay * dt);
                // (the solve's next operand is the ORCA wavefronts' float; (float)vel would give the same bits)
                vel = make_double2(hax, hay);
            }
            if (pop) s_hpos[hs] = pos;
            if (!restart) {
                if (track && htime == 0 && norm2(pos.x - goal.x, pos.y - goal.y) < rad) htime = t_new;
            }
            if (any_restart) {
                if (pop && restart) s_hrad[hs] = rad;
            }
        }

        long a2 = a, e2 = e;
        asm volatile("" : "+v"(a2), "+v"(e2));
        const KernargPtr kp = kernarg_here();
        if (active) {
            reinterpret_cast<double2 *>(kp->st.hpos)[a2] = pos;
            reinterpret_cast<double2 *>(kp->st.hvel)[a2] = vel;
            if (do_reset) {
                reinterpret_cast<double2 *>(kp->st.hgoal)[a2] = goal;
                kp->st.hrad[a2] = rad;
                kp->st.hvpref[a2] = vpref;
            }
            double *human_times = kp->st.human_times, *human_act = kp->out.human_act;
            if (human_times) human_times[a2] = htime;
            if (human_act) reinterpret_cast<double2 *>(human_act)[a2] = make_double2(hax, hay);
        }
        if (lead) {
            reinterpret_cast<double2 *>(kp->st.rpos)[e2] = rpos;
            reinterpret_cast<double2 *>(kp->st.rvel)[e2] = rvel;
            if (do_reset) reinterpret_cast<double2 *>(kp->st.rgoal)[e2] = rgoal;
            double *rth = kp->st.rtheta;
            if (rth) rth[e2] = rtheta;
            kp->st.gtime[e2] = gtime;
            store_step_rec(kp->out.rec + e2, o_rew, o_dmin, o_dn, o_inf, o_hh);
            if (has_state) kp->roll.state[e2] = rs;
        }
    }
    STAMP(39);
}

// The four-wavefront form as a kernel of its own: 256 lanes, two workgroups per CU.  (StepParams stays argument 0:
// kernarg_here.)
template <int NT, int VIS, bool UNI>
__global__ __launch_bounds__(256, 2) void env_rollout_wg4_kernel(const StepParams p, const int T)
{
    rollout_wg4<NT, VIS, UNI>(p, T);
}

void launch_env_rollout_wg4(const StepParams &p, int T, hipStream_t stream)
{
    constexpr int NT = 5, EW = Wg4<NT>::EW;
    const dim3 grid((p.E + EW - 1) / EW), block(256);
    if (p.cfg.robot_kinematics == MCN_KIN_UNICYCLE)
        hipLaunchKernelGGL((env_rollout_wg4_kernel<NT, 0, true>), grid, block, 0, stream, p, T);
    else
        hipLaunchKernelGGL((env_rollout_wg4_kernel<NT, 0, false>), grid, block, 0, stream, p, T);
}

#ifdef MCN_DIAG
int read_counts_wg4(void *dst, size_t bytes, int reset) { return read_counts_here(dst, bytes, reset); }
int read_stamps_wg4(void *dst, size_t bytes) { return read_stamps_here(dst, bytes); }
#endif

}  // namespace mcn
