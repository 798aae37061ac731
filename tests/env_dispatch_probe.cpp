// env_dispatch_probe.cpp -- csrc/env_dispatch.hpp from the outside, with the host compiler alone (no HIP, no GPU):
// reads one problem per line from stdin, prints its plan (tests/test_env_dispatch_cpu.py holds the expected table).
//
// A line is a list of key=value words (integers); anything left out keeps its default:
//   T       0: mcn_env_step / mcn_env_step_sf, > 0: mcn_env_rollout / mcn_env_rollout_sf of T steps        (0)
//   policy  MCN_HUMANS_*: 0 ORCA, 1 linear, 2 given velocities, 3 social force                                (0)
//   E N vis uni maxn update hh                                   (1, 5, 0, 0, 10, 1, 0)
//   queue   mcn_env_out.lp3_queue given            times  track_human_times with a human_times array
//   hact    mcn_env_out.human_act given            disc   mcn_rollout with a state and a discount table of this length
//   fg qmax qsplit rfused rsplit block pstream defer          mcn_tuning, as mcn_set_tuning(NULL) leaves it
// Output: family form quad_split block static_n lp3_defer pair_nontemporal; the five step fields are those of the
// single steps (all 0 when one launch takes the whole rollout).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include "../modelcrowdnav_amd/csrc/env_dispatch.hpp"

int main()
{
    static double buffer[4];                      // stands for "this optional array was given"; never dereferenced
    std::string line;
    while (std::getline(std::cin, line)) {
        std::map<std::string, int> v = {{"T", 0}, {"policy", 0}, {"E", 1}, {"N", 5}, {"vis", 0}, {"uni", 0},
                                        {"maxn", 10}, {"update", 1}, {"hh", 0}, {"queue", 0}, {"times", 0},
                                        {"hact", 0}, {"disc", 0}, {"fg", 0}, {"qmax", -1}, {"qsplit", -1},
                                        {"rfused", -1}, {"rsplit", -1}, {"block", -1}, {"pstream", -1}, {"defer", -1}};
        std::istringstream words(line);
        std::string w;
        bool any = false;
        while (words >> w) {
            const size_t eq = w.find('=');
            if (eq == std::string::npos || !v.count(w.substr(0, eq))) {
                std::fprintf(stderr, "unknown word '%s'\n", w.c_str());
                return 2;
            }
            v[w.substr(0, eq)] = std::atoi(w.c_str() + eq + 1);
            any = true;
        }
        if (!any) continue;
        mcn::StepParams p;
        std::memset(&p, 0, sizeof(p));
        p.cfg.time_step = 0.25;
        p.cfg.human_policy = v["policy"];
        p.cfg.robot_visible = v["vis"];
        p.cfg.robot_kinematics = v["uni"] ? MCN_KIN_UNICYCLE : MCN_KIN_HOLONOMIC;
        p.cfg.orca_max_neighbors = v["maxn"];
        p.cfg.count_hh = v["hh"];
        p.cfg.track_human_times = v["times"];
        p.st.human_times = v["times"] ? buffer : nullptr;
        p.out.lp3_queue = v["queue"] ? buffer : nullptr;
        p.out.human_act = v["hact"] ? buffer : nullptr;
        if (v["disc"] > 0) {
            p.has_roll = 1;
            p.roll.state = reinterpret_cast<mcn_roll_rec *>(buffer);
            p.roll.disc_table = buffer;
            p.roll.disc_len = v["disc"];
        }
        p.E = v["E"]; p.N = v["N"]; p.G = 64 / p.N; p.update = v["update"];
        mcn_tuning tu;
        std::memset(&tu, 0, sizeof(tu));
        tu.force_generic = v["fg"]; tu.quad_max_envs = v["qmax"]; tu.quad_split = v["qsplit"];
        tu.rollout_fused = v["rfused"]; tu.rollout_split = v["rsplit"]; tu.step_block = v["block"];
        tu.pair_stream = v["pstream"]; tu.lp3_defer = v["defer"]; tu.sarl_x3 = -1;
        mcn::KernelFamily family;
        mcn::StepPlan s = {};
        int form = -1;
        if (v["T"] > 0) {
            const mcn::RolloutPlan r = mcn::plan_env_rollout(p, v["T"], tu);
            family = r.family; form = r.form; s = r.step;
        } else {
            s = mcn::plan_env_step(p, tu);
            family = s.family;
        }
        std::printf("%s %d %d %d %d %d %d\n", mcn::family_name(family), form, s.quad_split ? 1 : 0, s.block,
                    s.static_n ? 1 : 0, s.lp3_defer ? 1 : 0, s.pair_nontemporal ? 1 : 0);
    }
    return 0;
}
