// Stand-alone check of the flow output's host side (netgauze_amd/csrc/ngz_output_plan.cpp), built
// with -fsanitize=address,undefined by tests/test_output_plan_native.py: builds a config of every
// select, plans a template record at every truncated length from exact-size heap copies (a read past
// the record is a sanitizer report), refuses a bad config, and prints what it got.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../netgauze_amd/csrc/ngz_output_plan.h"

int main() {
    const ngz_output_ref one[] = {{0, 8, 0}}, co[] = {{0, 11, 0}, {0, 7, 0}}, multi[] = {{0, 316, 0}, {0, 71, 0}, {0, 79, 0}},
                         l2[] = {{0, 351, 0}}, rep[] = {{0, 1, 1}};
    const uint8_t dflt[] = {'n', '/', 'a'};
    ngz_output_field f[5];
    memset(f, 0, sizeof f);
    f[0].name = "ip"; f[0].refs = one; f[0].n_refs = 1; f[0].default_kind = NGZ_OUT_DEF_STRING; f[0].default_bytes = dflt; f[0].default_len = 3;
    f[1].name = "port"; f[1].select = NGZ_OUT_SEL_COALESCE; f[1].refs = co; f[1].n_refs = 2;
    f[2].name = "mpls"; f[2].select = NGZ_OUT_SEL_MULTI; f[2].transform = NGZ_OUT_TR_MPLS_INDEX; f[2].refs = multi; f[2].n_refs = 3;
    f[3].name = "vni"; f[3].select = NGZ_OUT_SEL_L2SEGMENT; f[3].encap_type = 1; f[3].refs = l2; f[3].n_refs = 1;
    f[4].name = "bytes2"; f[4].refs = rep; f[4].n_refs = 1; f[4].transform = NGZ_OUT_TR_STRING;
    ngzout::Config cfg;
    std::string err;
    if (ngzout::build_config(f, 5, &cfg, &err)) return 1;
    printf("%s\n", ngzout::schema_text(cfg).c_str());
    // options template 300: 2 scope fields (1, 8), then 1, 7, 71, 351, 1
    const uint8_t rec[] = {1, 44, 0, 7, 0, 2, 0, 1, 0, 8, 0, 8, 0, 4, 0, 1, 0, 8, 0, 7, 0, 2, 0, 71, 0, 3, 1, 95, 0, 8, 0, 1, 0, 8};
    for (size_t len = 0; len <= sizeof rec; ++len) {
        uint8_t *copy = new uint8_t[len ? len : 1];
        memcpy(copy, rec, len);
        ngz_output_plan p;
        const int rc = ngzout::template_plan(cfg, copy, len, 10 | NGZ_OUTPUT_OPTIONS, &p);
        delete[] copy;
        if ((rc == 0) != (len == sizeof rec)) return 2;
        if (rc) continue;
        for (uint32_t i = 0; i < p.n_fields; ++i) {
            printf("F%u t%u n%u :", i, p.f[i].avro_type, p.f[i].nullable);
            for (uint32_t s = 0; s < p.f[i].n_present; ++s) printf(" %d", p.f[i].src[s]);
            printf("\n");
        }
    }
    f[1].n_refs = 0;
    const int rc = ngzout::build_config(f, 5, &cfg, &err);
    printf("R %d %s\n", rc, err.c_str());
    return rc == NGZ_OUTPUT_E_CONFIG ? 0 : 3;
}
