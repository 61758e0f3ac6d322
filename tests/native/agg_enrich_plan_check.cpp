// Stand-alone check of the aggregation-over-enrichment planner
// (netgauze_amd/csrc/ngz_agg_enrich_plan.cpp), built with -fsanitize=address,undefined by
// tests/test_agg_enrich_plan_native.py: resolves every query of the file named on the command line
// and prints the resolutions.
//   Q <n_fields> {<pen> <ie> <is_scope>} <n_cols> {<pen> <ie> <index>} <pen> <ie> <index>
#include <cstdio>
#include <fstream>
#include <string>

#include "ngz/flow_aggregate.h"

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    std::string tag;
    while (in >> tag) {
        unsigned nf, nc, pen, ie, index;
        in >> nf;
        // exact-size heap copies: a read past either list is a sanitizer report
        ngz_agg_slot_field *f = new ngz_agg_slot_field[nf ? nf : 1];
        for (unsigned i = 0; i < nf; ++i) {
            unsigned p, e, s;
            in >> p >> e >> s;
            f[i] = ngz_agg_slot_field{p, (uint16_t)e, (uint8_t)s, 0};
        }
        in >> nc;
        ngz_agg_ref *c = new ngz_agg_ref[nc ? nc : 1];
        for (unsigned i = 0; i < nc; ++i) {
            unsigned p, e, x;
            in >> p >> e >> x;
            c[i] = ngz_agg_ref{p, (uint16_t)e, (uint16_t)x};
        }
        in >> pen >> ie >> index;
        ngz_agg_enrich_resolution r;
        const int rc = ngz_agg_enrich_field_plan(nf ? f : nullptr, nf, nc ? c : nullptr, nc, pen, (uint16_t)ie, (uint16_t)index, &r);
        delete[] f;
        delete[] c;
        printf("R %d", rc);
        if (rc == 0) {
            printf(" %u %u %u %u %u %u |", r.kind, r.dropped, r.kind == NGZ_AGG_RES_OWN ? r.own_field : 0u, r.n_candidates,
                   r.ordinal, r.writer_after);
            for (unsigned i = 0; i < r.n_candidates; ++i) printf(" %u", r.candidates[i]);
        }
        printf("\n");
    }
    return 0;
}
