// env_rollout_wg4.hip -- the four-wavefront form of the fused T-step rollout (env_rollout_quad.hip has the other two and the
// dispatch): 8 envs x 5 humans per workgroup, three float32 ORCA wavefronts and one float64 wavefront.  A translation unit
// of its own because it is built WITHOUT the SLP vectoriser (Makefile): the packed float32 instructions the vectoriser
// forms in the ORCA solve cost a wavefront that shares its SIMD 8.75 cycles each, plus the moves that pair their operands,
// and the scalar instructions they stand for 4.6 - 5.0 (profiles/r04_valu_issue.txt, profiles/r18_orca_issue.txt).  The
// other forms keep the flags, and so the code, they had.
#include "env_rollout_common.hpp"

namespace mcn {

// Four-wavefront form (env_rollout_wg4_kernel): workgroups of EW envs on FOUR wavefronts -- three ORCA wavefronts
// for the EW * NT quads, dealt in order
// (quad q = env q / NT, human q % NT, so an env may straddle two wavefronts), and one float64 wavefront with eight
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
// from the pool by it, stored in its epilogue.  The ORCA wavefronts are float32 only: per step they read their human's
// operands and their candidate's from LDS (what and when: below), run quad_orca_core (quad_common.hpp) and publish the new velocity as two
// floats.  The four lanes of a quad would each repeat the float64 -> float32 conversions, the integrate and the restart
// test; the float64 wavefront does them once per human and has the cycles to spare, and on a SIMD that holds two
// wavefronts every instruction taken out of the ORCA stream is taken out of its neighbour's way too.
// The roles meet through LDS at two points of the step: hand-off 1, ORCA -> float64, the new velocities; hand-off 2,
// float64 -> ORCA, the new positions (the float64 wavefront integrates between the two).  Between the two all four
// wavefronts wait for one serial chain, so only what depends on the new velocity is on it: read (rx, ry), two
// conversions, the integrate, goal - pos, four conversions, one 16-byte write.  Everything else stays off it:
//   * the velocity never leaves float32: the solve's velocity operands are the floats the ORCA wavefronts produced
//     (float32 -> float64 -> float32 gives the same bits back): the owner's are the (rx, ry) its quad still holds, the
//     candidate's are read from s_res;
//   * frad and the maximum speed change only on a restart and live in s_inv, written in the prologue and by restart lanes;
//     the ORCA wavefronts keep them, and the candidate's frad, in registers from one restart step to the next;
//   * what a restarted human publishes (position pack, start velocity, s_inv) is converted BEFORE hand-off 1, where the
//     float64 wavefront would idle anyway, and stored between the hand-offs behind one wave-uniform branch;
//   * the float64 wavefront's private arrays, its register update and the human_times test come after hand-off 2.
// Each value is produced by the operation, on the operands, that the other forms use, so the same bits.
//
// The top of an ORCA wavefront's step reads only what hand-off 2 published, the two position packs.  Everything else the
// solve needs is final at hand-off 1 and is fetched or kept: the candidate's velocity is read
// BETWEEN the hand-offs, where the ORCA wavefronts wait for the float64 chain anyway -- except on a restart step, when a
// restart lane overwrites its human's velocity and s_inv inside that very interval.  The float64 wavefront knows
// any_restart when its ladder ends and stores it to s_flag[0] there; the ORCA wavefronts read it between the hand-offs,
// make it a scalar, and on a restart step (and on step 0 of every launch, whose operands the prologue seeded) take the
// SLOW PATH behind hand-off 2: own and candidate's velocity, (frad, ms) and the candidate's frad from LDS.  s_res is one
// buffer, so those reads are fenced from the next solves' writes by a THIRD BARRIER, which all four wavefronts execute
// on such steps and no other: the float64 wavefront branches on its own any_restart (and the prologue's second barrier
// stands for step 0), the ORCA wavefronts on the flag it stored, so every wavefront counts the same barriers (after the
// launch's last step the ORCA wavefronts execute it behind their loop, with nothing to read).
// The three intervals of a step and who touches what in them (W = writes, R = reads; f64 = the float64 wavefront):
//   A  hand-off 2 of the step before (or the prologue's barriers) -> hand-off 1: the solve
//   B  hand-off 1 -> hand-off 2: the float64 chain
//   C  restart steps only: hand-off 2 -> the third barrier (the head of the next step's interval A)
//              A                                   B                                        C
//   s_pack     R ORCA (top of step)                W f64 (every lane; restart lanes theirs)  R ORCA (it is their top of step)
//   s_res      W ORCA (end of solve)               R f64, R ORCA (candidate), W f64 restart  R ORCA (own, candidate)
//   s_inv      --                                  W f64 restart lanes                       R ORCA (own, candidate)
//   s_flag     W f64 (behind its ladder)           R ORCA                                    --
//   s_hpos/s_hrad  R f64 (pairs); W f64 (head of A: behind hand-off 2 / the third barrier)   --  (its own arrays)
//   s_lines    W/R the owning ORCA wavefront       --                                        --
// The candidate's velocity an ORCA wavefront reads in B of a restart step races with the restart lane's write; that value
// is never used: the slow path overwrites it in C.  In C the ORCA wavefronts wait for
// their reads before the third barrier, and the first write of s_res behind it is the end of the next solve.
//
// The float64 wavefront's ladder, Explorer accounting, finished-episode stores, robot integrate / restart and the epilogue
// are the TWIN of env_rollout_quad_kernel's (env_rollout_quad.hip): a change to either is made to both.  The text is
// not shared: with the tail in common functions this kernel's two forms came out at 1791 and 2811 instructions for
// 1804 and 2840 with another SGPR use, and the older kernel lost registers to scratch (profiles/r19_env_refactor.txt,
// section 4), on the path the benchmark's headline runs.  The humans' integrate / restart holds the twin's statements
// (pos + (double)r * dt, the pool fetch, human_times) in another order: the restart before hand-off 1, the integrate
// between the hand-offs, the velocity register and human_times after hand-off 2.
template <int NT>
struct Wg4 {
    static_assert(NT == 5, "the four-wavefront form is built for 5 humans only");
    static constexpr int EW = 8;                              // envs per workgroup
    static constexpr int NQ = EW * NT;                        // populated quads = populated float64 lanes: 40 of 48 / 64
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

template <int NT, int VIS, bool UNI>
__device__ __forceinline__ void rollout_wg4(const StepParams &p, const int T)
{
    static_assert(VIS == 0, "the four-wavefront form is built for an invisible robot only");
    constexpr int EW = Wg4<NT>::EW, NQ = Wg4<NT>::NQ;
    // hand-off arrays, one slot per (env, human).  Written by the float64 wavefront between the step's two barriers:
    // s_pack = (px, py, prefx, prefy) of quad_orca_core's operands, every step; s_inv = (frad, maximum speed) and the
    // start velocity in s_res, restart lanes only.  Written by the ORCA wavefronts outside that window, read by the
    // float64 one and (their candidate's) by the ORCA ones inside it, and by the ORCA ones' slow path behind it: s_res,
    // the human's new velocity, one buffer (table above).  s_hpos / s_hrad, the float64 position and radius the overlap
    // pairs read from partner lanes, are the float64 wavefront's own: written after the second barrier, read in its
    // next step.
    __shared__ float4 s_pack[NQ];
    __shared__ float2 s_res[NQ], s_inv[NQ];
    // word 0: some human of the workgroup restarts on this step (the float64 wavefront's any_restart).  The other words
    // are the room the second velocity buffer had: the workgroup's LDS, and with it the CU's, stays what it was
    __shared__ int s_flag[2 * NQ];
    __shared__ double2 s_hpos[NQ];
    __shared__ double s_hrad[NQ];
    // the ORCA wavefronts' sorted half-planes (quad_common.hpp: QuadTable): 64 slots each, private to the wavefront.  A lane
    // reads its quad's four slots, its own, and the two operands of its pass-A intersection (lp1_spread): seven reads
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
        // ---------------- ORCA wavefronts: the float32 solve, nothing else ----------------
        const int lane = tid & 63, k = tid & 3, q = tid >> 2;
        const bool pop = q < NQ;                                 // idle quads (and envs >= E) hold no half-plane, write nothing
        const int ge = q / NT, h = q - ge * NT;
        const bool active = pop && (long)chunk_ * EW + ge < p.E;
        const int hi = pop ? q : 0;                              // LDS slot of this quad's human (idle quads read slot 0)
        const bool cand_h = k < NT - 1;                          // candidate is another human
        const int j = cand_h ? k + (k >= h ? 1 : 0) : h;
        const int ci = pop ? ge * NT + j : 0;
        const bool publish = pop && k == 0;
        const float inv_th = in_vgpr(1.0f / c.orca_time_horizon), inv_ts = in_vgpr(1.0f / (float)c.time_step);
        float4 *const tab = s_lines + role * 64;
        // what a normal step keeps in registers: own velocity v, the candidate's cv, (frad, ms) and the candidate's frad
        float vx = 0, vy = 0, cvx = 0, cvy = 0, frad = 0, ms = 0, orad = 0;
        bool slow = true;                                        // wave-uniform: step 0 of a launch is a restart step
        __syncthreads();                                         // the float64 wavefront has seeded the packs
        STAMP(1);

        for (int t = 0; t < T; ++t) {
            // behind hand-off 2: the positions, own and candidate's, on every step
            float4 P = s_pack[hi];
            float2 cp = *reinterpret_cast<const float2 *>(s_pack + ci);
            if (slow) {
                // restart step (and step 0): every other operand from LDS too -- the velocities as the prologue or
                // the last step's solves left them with restart lanes overwritten, frad / ms as the restart lanes left
                // them.  Issued behind the two above, one LDS round trip for the six: the empty asm needs the last four,
                // and LDS answers in order.  (The positions stay out of it: as its operands they would be copied into
                // the registers the two paths share, six moves on every normal step.)  The barrier behind it keeps the
                // solves' next write of s_res behind every wavefront's reads.
                float2 v = s_res[hi], cv = s_res[ci];
                float2 fm = s_inv[hi];
                float od = s_inv[ci].x;                          // the candidate's own frad
                asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(cv.x), "+v"(cv.y), "+v"(fm.x), "+v"(fm.y), "+v"(od));
                __syncthreads();                                 // restart steps only: s_res has been read
                vx = v.x; vy = v.y; cvx = cv.x; cvy = cv.y; frad = fm.x; ms = fm.y; orad = od;
            }
            float rx, ry;
            quad_orca_core(c, lane, k, cand_h && active, make_float4(P.x, P.y, vx, vy), make_float4(P.z, P.w, frad, ms),
                           make_float4(cp.x, cp.y, cvx, cvy), orad, inv_th, inv_ts, rx, ry, QuadTable{tab});
            if (publish) s_res[hi] = make_float2(rx, ry);
            if (t < 20) STAMP(40 + t);
            __syncthreads();                                     // hand-off 1: the humans' new velocities
            // between the hand-offs, where this wavefront waits for the float64 chain: the workgroup's restart flag and
            // the candidate's new velocity, one LDS round trip; the own new velocity is (rx, ry), identical on the
            // quad's lanes.  On a restart step the candidate's read races with the restart lane's overwrite and the quad's
            // registers hold the old human's: nothing formed here is used then, the slow path re-reads it all.
            int flag = s_flag[0];
            float2 cv = s_res[ci];
            asm volatile("" : "+v"(flag), "+v"(cv.x), "+v"(cv.y));      // waited for before the barrier
            slow = __builtin_amdgcn_readfirstlane(flag) != 0;
            vx = rx; vy = ry; cvx = cv.x; cvy = cv.y;
            __syncthreads();                                     // hand-off 2: the next step's positions
            if (t < 37) STAMP(2 + t);
        }
        // the float64 wavefront executes the third barrier of the last step too (no test of the step count in its loop)
        if (slow) __syncthreads();
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
        // the first step's operands: the loaded state goes through the hand-off arrays
        {
            float4 A, B;
            quad_orca_operands(c, pos, vel, goal, rad, vpref, A, B);
            if (pop) {
                s_pack[hs] = make_float4(A.x, A.y, B.x, B.y); s_res[hs] = make_float2(A.z, A.w);
                s_inv[hs] = make_float2(B.z, B.w);
                s_hpos[hs] = pos; s_hrad[hs] = rad;
            }
        }
        __syncthreads();
        __syncthreads();                                         // step 0 is a restart step: the ORCA wavefronts have read s_res
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
            // wavefront reaches hand-off 1 (issued there, the barrier's wait for it sat on the chain of every step on
            // which this wavefront is the last to arrive: the unicycle robot's)
            const bool restart = do_reset && dn;
            const bool any_restart = __any(restart);             // roughly one workgroup-step in ten
            s_flag[0] = any_restart ? 1 : 0;                     // (every lane the same word: no exec mask to set up)

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

            // ---- humans of a finished env restart from the scenario pool NOW, while this wavefront would wait at hand-off 1
            //      for the ORCA ones anyway (it knows the done flag first): the case is fetched straight into the state
            //      registers (nothing below reads the old one: the swept circle, the pairs and the ladder are done) and
            //      converted; between the hand-offs a restart lane only stores what it holds here ----
            float4 n_pack = make_float4(0, 0, 0, 0);
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
                // every float converted from the new float64 state, as the prologue does for a loaded one
                float4 A, B;
                quad_orca_operands(c, pos, vel, goal, rad, vpref, A, B);
                // (pinned: not to be sunk behind the barrier)
                n_pack = make_float4(in_vgpr(A.x), in_vgpr(A.y), in_vgpr(B.x), in_vgpr(B.y));
                n_fvel = make_float2(in_vgpr(A.z), in_vgpr(A.w));
                n_inv = make_float2(in_vgpr(B.z), in_vgpr(B.w));
            }

            if (t < 20) STAMP(40 + t);
            __syncthreads();                                     // hand-off 1: the humans' new velocities
            // ---- the chain every wavefront of the workgroup waits for: velocity -> position -> pack ----
            float2 *vel_io = s_res;
            {
                const float2 r = vel_io[hs];
                hax = (double)r.x; hay = (double)r.y;            // (restart lanes too: the epilogue's human_act)
            }
            if (!restart) {
                pos = make_double2(pos.x + hax * dt, pos.y + hay * dt);
                if (pop) s_pack[hs] = quad_orca_position_pack(pos, goal);
            }
            if (any_restart) {                                   // (stores under their own mask: no select on the chain)
                if (pop && restart) { s_pack[hs] = n_pack; vel_io[hs] = n_fvel; s_inv[hs] = n_inv; }
            }
            __syncthreads();                                     // hand-off 2: the next step's positions
            // restart steps only: the ORCA wavefronts re-read every operand behind hand-off 2 and fence those reads from
            // their solves' next write of s_res with one more barrier (after the last step: behind their loop); this
            // wavefront takes part at once, before its own work, on its own copy of the flag they read
            if (any_restart) __syncthreads();
            if (t < 37) STAMP(2 + t);

            // ---- off the chain: this wavefront's own arrays, the velocity register, the clock of the step just taken ----
            if (pop) s_hpos[hs] = pos;
            if (!restart) {
                // (the solve's next operand is the ORCA wavefronts' float; (float)vel would give the same bits)
                vel = make_double2(hax, hay);
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
