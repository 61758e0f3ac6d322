// Stand-alone check of the host enrichment cache (netgauze_amd/csrc/ngz_enrich_cache.cpp), built
// with -fsanitize=address,undefined by tests/test_enrich_cache_native.py: replays a script of
// operations and lookups from the file named on the command line and prints the results.
//   O <kind> <ip: family + 16 bytes, hex> <domain> <weight> <n scope> <n fields> <n ies>
//   F <pen> <ie> <kind> <value hex or ->        (scope fields, then fields)
//   I <pen> <ie>
//   L <ip> <domain> <n record fields>, then F lines
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "ngz_enrich_cache.h"

static std::string unhex(const std::string &h) {
    std::string out;
    if (h == "-") return out;
    for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((char)std::stoi(h.substr(i, 2), nullptr, 16));
    return out;
}

struct Fields {
    std::vector<std::string> bytes;
    std::vector<ngz_enrich_field> f;
    void read(std::istream &in, size_t n) {
        bytes.resize(n);
        f.assign(n, ngz_enrich_field{});
        for (size_t i = 0; i < n; ++i) {
            std::string tag, hex;
            unsigned pen, ie, kind;
            in >> tag >> pen >> ie >> kind >> hex;
            bytes[i] = unhex(hex);
            f[i].pen = pen;
            f[i].ie_id = (uint16_t)ie;
            f[i].kind = (uint8_t)kind;
            f[i].len = (uint32_t)bytes[i].size();
        }
        for (size_t i = 0; i < n; ++i) f[i].value = (const uint8_t *)bytes[i].data();
    }
};

static ngz_enrich_peer peer_of(const std::string &hex) {
    const std::string b = unhex(hex);
    ngz_enrich_peer p{};
    p.family = (uint8_t)b[0];
    for (int i = 0; i < 16; ++i) p.addr[i] = (uint8_t)b[1 + i];
    return p;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    ngze::Cache cache;
    std::string tag;
    while (in >> tag) {
        if (tag == "O") {
            unsigned kind, domain, weight, ns, nf, ni;
            std::string ip;
            in >> kind >> ip >> domain >> weight >> ns >> nf >> ni;
            Fields scope, fields;
            scope.read(in, ns);
            fields.read(in, nf);
            std::vector<ngz_enrich_ie> ies(ni);
            for (unsigned i = 0; i < ni; ++i) {
                std::string t;
                unsigned pen, ie;
                in >> t >> pen >> ie;
                ies[i] = ngz_enrich_ie{pen, (uint16_t)ie, 0};
            }
            ngz_enrich_operation op{};
            op.kind = (uint8_t)kind;
            op.weight = (uint8_t)weight;
            op.peer = peer_of(ip);
            op.obs_domain_id = domain;
            op.n_scope = ns; op.n_fields = nf; op.n_ies = ni;
            op.scope = scope.f.data(); op.fields = fields.f.data(); op.ies = ies.data();
            std::string why;
            const int rc = cache.apply(op, &why);
            printf("P %d %llu %llu\n", rc, (unsigned long long)cache.peer_count(), (unsigned long long)cache.generation());
        } else if (tag == "L") {
            std::string ip;
            unsigned domain, n;
            in >> ip >> domain >> n;
            Fields rec;
            rec.read(in, n);
            ngze::PeerIp key;
            const ngz_enrich_peer p = peer_of(ip);
            ngze::peer_ip(&p, &key);
            const std::vector<ngze::Resolved> r = cache.lookup(key, domain, rec.f.data(), n);
            printf("R %zu\n", r.size());
            for (const ngze::Resolved &x : r) {
                printf("%u %u %u %u %u ", x.ref.pen, x.ref.ie, x.ref.index, x.field->value.kind, x.field->weight);
                if (x.field->value.bytes.empty()) printf("-");
                for (unsigned char c : x.field->value.bytes) printf("%02x", c);
                printf("\n");
            }
        }
    }
    return 0;
}
