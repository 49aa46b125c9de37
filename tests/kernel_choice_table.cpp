// Driver of tests/test_kernel_choice.py: every argument is one row "facts|env" of the kernel-choice table; for each the driver
// sets the process environment, reads it back through read_choice_env() and prints kernel_name(choose_kernel(...)), a tab and
// arith_covered.  Facts: a base row (F0, G0, nvdb) followed by changes; env: NAME or NAME=VALUE without the VSPG_ prefix.
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include <vector>

#include "vspg_kernel_choice.h"

using namespace vspg_choice;

static const char *const kEnvNames[] = {"VSPG_KERNEL", "VSPG_WG_SCHED", "VSPG_NO_GREY_GUIDED", "VSPG_WF_MERGED"};

static std::vector<std::string> split(const std::string &s, char sep) {
    std::vector<std::string> out;
    std::stringstream ss(s);
    for (std::string item; std::getline(ss, item, sep);) out.push_back(item);
    return out;
}

static bool apply_fact(ChoiceFacts &f, const std::string &t) {
    if (t == "F0" || t == "G0" || t == "nvdb") {
        // F0: homogeneous medium, no triangles, infinite lights, spheres or boundaries, uniform light sampler, all three grey flags,
        // unguided, resampling, no tr_calc, no temperature.  G0 / nvdb: as F0 over a grid / NanoVDB medium, medium_grey false.
        f = ChoiceFacts();
        f.medium_type = t == "F0" ? VSPG_MEDIUM_HOMOGENEOUS : t == "G0" ? VSPG_MEDIUM_GRID : VSPG_MEDIUM_NANOVDB;
        f.medium_grey = t == "F0";
        f.surfaces_grey = f.null_zero = true;
    } else if (t == "null_zero=0") f.null_zero = false;
    else if (t == "surfaces_grey=0") f.surfaces_grey = false;
    else if (t == "medium_grey=0") f.medium_grey = false;
    else if (t == "medium_grey=1") f.medium_grey = true;
    else if (t == "n_tris>0") f.n_tris = 12;
    else if (t == "n_inf>0") f.n_inf = 1;
    else if (t == "n_spheres>0") f.n_spheres = 1;
    else if (t == "power") f.lightsampler = VSPG_LIGHTSAMPLER_POWER;
    else if (t == "boundaries") f.has_boundaries = true;
    else if (t == "guided") f.guided = true;
    else if (t == "rrguiding") f.rrguiding = true;
    else if (t == "training") f.training = true;
    else if (t == "tr_calc") f.tr_calc = true;
    else if (t == "temperature") f.has_temperature = true;
    else if (t == "not resampling") f.resampling = false;
    else return false;
    return true;
}

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) {
        const std::string row = argv[i];
        const size_t bar = row.find('|');
        if (bar == std::string::npos) { fprintf(stderr, "row without '|': %s\n", argv[i]); return 2; }
        ChoiceFacts f;
        for (const std::string &t : split(row.substr(0, bar), ','))
            if (!apply_fact(f, t)) { fprintf(stderr, "unknown fact '%s' in row %s\n", t.c_str(), argv[i]); return 2; }
        for (const char *n : kEnvNames) unsetenv(n);
        for (const std::string &t : split(row.substr(bar + 1), ',')) {
            const size_t eq = t.find('=');
            const std::string name = "VSPG_" + t.substr(0, eq);
            bool known = false;
            for (const char *n : kEnvNames) known = known || name == n;
            if (!known) { fprintf(stderr, "unknown variable '%s' in row %s\n", name.c_str(), argv[i]); return 2; }
            setenv(name.c_str(), eq == std::string::npos ? "1" : t.substr(eq + 1).c_str(), 1);
        }
        const KernelChoice c = choose_kernel(f, read_choice_env());
        printf("%s\t%d\n", kernel_name(c).c_str(), c.arith_covered ? 1 : 0);
    }
    return 0;
}
