// knobs_check.cpp -- read_knobs() (gpusimilarity_amd/csrc/capi_knobs.cpp) against recorded values: for every line "name, unset | set,
// string, value" of the table given as argv[1], with no other knob in the environment, the knob's member reads `value`.  Every knob
// of the table read_knobs walks, and the two it reads by hand, must have lines.  tests/test_knobs_host.py builds and runs it with
// tests/golden/knobs_parse.tsv.  No GPU, no HIP runtime: it links the knobs' translation unit alone.
#include "../../gpusimilarity_amd/csrc/capi_knobs.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <set>
#include <string>
#include <vector>

using namespace gsim_host;

static bool value_of(const Knobs& k, const std::string& name, long long* out)
{
    for (size_t i = 0; i < kKnobSpecCount; i++)
        if (name == kKnobSpecs[i].name) return *out = k.*kKnobSpecs[i].member, true;
    if (name == "GSIM_DEBUG_BATCH") return *out = k.debug_batch, true;
    if (name == "GSIM_FOLD_RESCORE") return *out = k.fold_rescore_host, true;
    return false;
}

int main(int argc, char** argv)
{
    if (argc != 2) return std::fprintf(stderr, "usage: knobs_check TABLE.tsv\n"), 2;
    std::ifstream in(argv[1]);
    if (!in) return std::fprintf(stderr, "cannot read %s\n", argv[1]), 2;
    std::vector<std::string> names{"GSIM_DEBUG_BATCH", "GSIM_FOLD_RESCORE"};
    for (size_t i = 0; i < kKnobSpecCount; i++) names.push_back(kKnobSpecs[i].name);
    for (const std::string& n : names) unsetenv(n.c_str());
    std::set<std::string> seen;
    std::string line;
    int bad = 0, lines = 0;
    while (std::getline(in, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::vector<std::string> f; // name, unset | set, string, value
        for (size_t at = 0;;) {
            const size_t tab = line.find('\t', at);
            f.push_back(line.substr(at, tab == std::string::npos ? tab : tab - at));
            if (tab == std::string::npos) break;
            at = tab + 1;
        }
        if (f.size() != 4 || (f[1] != "set" && f[1] != "unset")) return std::fprintf(stderr, "malformed line: %s\n", line.c_str()), 2;
        if (f[1] == "set") setenv(f[0].c_str(), f[2].c_str(), 1);
        long long got = 0;
        const bool known = value_of(read_knobs(), f[0], &got);
        unsetenv(f[0].c_str());
        lines++;
        seen.insert(f[0]);
        if (!known || got != std::atoll(f[3].c_str())) {
            std::printf("%s %s \"%s\": %s, recorded %s\n", f[0].c_str(), f[1].c_str(), f[2].c_str(), known ? std::to_string(got).c_str() : "no such knob",
                        f[3].c_str());
            bad++;
        }
    }
    for (const std::string& n : names)
        if (!seen.count(n)) {
            std::printf("%s: no recorded lines\n", n.c_str());
            bad++;
        }
    if (bad) return std::printf("%d of %d lines differ\n", bad, lines), 1;
    std::printf("ok %d lines, %zu knobs\n", lines, names.size());
    return 0;
}
