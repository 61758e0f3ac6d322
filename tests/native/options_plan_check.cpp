// Stand-alone check of the flow-options planner (netgauze_amd/csrc/ngz_options_plan.cpp), built
// with -fsanitize=address,undefined by tests/test_options_plan_native.py: plans every template
// record of the file named on the command line and prints the plans.
//   T <proto> <options 0|1> <record hex or ->
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "ngz/flow_options.h"

static std::vector<uint8_t> unhex(const std::string &h) {
    std::vector<uint8_t> out;
    if (h == "-") return out;
    for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((uint8_t)std::stoi(h.substr(i, 2), nullptr, 16));
    return out;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    std::string tag, hex;
    int proto, options;
    while (in >> tag >> proto >> options >> hex) {
        // an exact-size heap copy: a read past the record is a sanitizer report
        const std::vector<uint8_t> rec = unhex(hex);
        uint8_t *copy = new uint8_t[rec.size() ? rec.size() : 1];
        for (size_t i = 0; i < rec.size(); ++i) copy[i] = rec[i];
        ngz_options_plan p;
        const int rc = ngz_options_template_plan(copy, rec.size(), proto | (options ? NGZ_OPTIONS_OPTIONS : 0), &p);
        delete[] copy;
        printf("P %d", rc);
        if (rc == 0) {
            printf(" %u %u %u %u", p.klass, p.outcome, p.n_ops, p.id_equal);
            for (unsigned o = 0; o < p.n_ops; ++o) {
                printf(" |");
                for (unsigned i = 0; i < p.n_scope[o]; ++i)
                    printf(" s%u.%u.%u@%u", p.scope[o][i].pen, p.scope[o][i].ie_id, p.scope[o][i].index, p.scope_src[o][i]);
                for (unsigned i = 0; i < p.n_fields[o]; ++i)
                    printf(" f%u.%u.%u@%u", p.fields[o][i].pen, p.fields[o][i].ie_id, p.fields[o][i].index, p.fields_src[o][i]);
            }
        }
        printf("\n");
    }
    return 0;
}
