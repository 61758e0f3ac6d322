// Stand-alone check of netgauze_amd/csrc/ngz_renorm_math.h on the host (tests/test_renorm_math_native.py
// builds it with -fsanitize=undefined,float-cast-overflow and compares every line with tests/renorm_ref.py).
// stdin, one record per line:  present v34 v35 v49 v50 v304 v305 v306 v309 v310 p311_bits(hex) count
// stdout:                      has_k k_bits(hex) new_count flag invalid inferred
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "ngz_renorm_math.h"

int main() {
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        NgzRenormParams p{};
        uint64_t bits = 0, count = 0;
        if (sscanf(line, "%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32
                         " %" SCNu32 " %" SCNu32 " %" SCNx64 " %" SCNu64,
                   &p.present, &p.interval34, &p.algorithm35, &p.mode49, &p.interval50, &p.selector304, &p.interval305,
                   &p.space306, &p.size309, &p.population310, &bits, &count) != 12) {
            fprintf(stderr, "bad line: %s", line);
            return 2;
        }
        memcpy(&p.probability311, &bits, 8);
        const NgzRenormFactor f = ngz_renorm_factor(p);
        uint64_t kb = 0;
        memcpy(&kb, &f.k, 8);
        const uint64_t out = f.has_k ? ngz_renorm_scale(count, f.k) : count;
        printf("%u %016" PRIx64 " %" PRIu64 " %u %u %u\n", f.has_k, f.has_k ? kb : 0, out, f.has_k, f.invalid, f.inferred);
    }
    return 0;
}
