// Stand-alone check of the template-record walker (netgauze_amd/csrc/ngz_template_record.h), built
// with -fsanitize=address,undefined by tests/test_template_record_native.py: walks every record of
// the file named on the command line and prints its specifiers, or the refusal.
//   T <proto> <options 0|1> <record hex or ->
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "ngz_template_record.h"

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
        // an exact-size heap copy: a read at or past the record's length is a sanitizer report
        const std::vector<uint8_t> rec = unhex(hex);
        uint8_t *copy = new uint8_t[rec.size()];
        for (size_t i = 0; i < rec.size(); ++i) copy[i] = rec[i];
        std::string line;
        const int rc = ngzt::walk_template_record(copy, rec.size(), proto, options != 0, [&](const ngzt::FieldSpec &f) {
            char buf[64];
            snprintf(buf, sizeof buf, " %c%u.%u.%u", f.scope ? 's' : 'f', f.pen, f.ie, f.length);
            line += buf;
        });
        delete[] copy;
        if (rc) printf("R %d\n", rc);
        else printf("F%s\n", line.c_str());
    }
    return 0;
}
