// The per-template plan of the flow-options input (ngz_options_plan.h).  Host only, no HIP.
#include "ngz_options_plan.h"

#include <cstring>
#include <map>
#include <utility>

#include "ngz_template_record.h"

namespace ngzo {
namespace {

enum : uint16_t {
    IE_ingressInterface = 10, IE_egressInterface = 14, IE_samplingInterval = 34, IE_samplerRandomInterval = 50,
    IE_interfaceName = 82, IE_interfaceDescription = 83, IE_mplsVpnRouteDistinguisher = 90, IE_lineCardId = 141,
    IE_exportingProcessId = 144, IE_paddingOctets = 210, IE_ingressVRFID = 234, IE_egressVRFID = 235, IE_VRFname = 236,
    IE_samplingPacketInterval = 305, IE_samplingPacketSpace = 306, IE_samplingTimeInterval = 307,
    IE_samplingTimeSpace = 308, IE_samplingSize = 309, IE_samplingPopulation = 310, IE_samplingProbability = 311,
};
constexpr uint32_t PEN_NETGAUZE = 3746;
constexpr uint16_t NO_SRC = 0xFFFF;

struct Item {  // a Field of the record as the reference sees it, and the template field its value comes from
    uint32_t pen;
    uint16_t ie;
    uint16_t src;
};
using Items = std::vector<Item>;

// FieldRefLookup::get_by_ie of one map (types.rs:164-174): occurrence index 0 is the first in order
const Item *first_of(const Items &v, uint16_t ie) {
    for (const Item &x : v)
        if (x.pen == 0 && x.ie == ie) return &x;
    return nullptr;
}

// One operation's list with its occurrence indices (FieldRef::map_fields, types.rs:82-100)
int emit(const Items &v, ngz_options_ref *refs, uint16_t *src, uint8_t *n) {
    if (v.size() > NGZ_OPTIONS_MAX_REFS) return NGZ_E_LIMIT;
    std::map<std::pair<uint32_t, uint16_t>, uint16_t> seen;
    for (size_t i = 0; i < v.size(); ++i) {
        refs[i].pen = v[i].pen;
        refs[i].ie_id = v[i].ie;
        refs[i].index = seen[{v[i].pen, v[i].ie}]++;
        src[i] = v[i].src;
    }
    *n = (uint8_t)v.size();
    return NGZ_OK;
}

}  // namespace

int plan_fields(const std::vector<PlanField> &fields, int proto, ngz_options_plan *out) {
    memset(out, 0, sizeof *out);
    out->id_src[0] = out->id_src[1] = NO_SRC;
    if (fields.size() >= NO_SRC) return NGZ_E_LIMIT;
    Items scope, rest;
    bool any_scope = false;
    for (size_t i = 0; i < fields.size(); ++i) {
        const PlanField &f = fields[i];
        const uint16_t src = (uint16_t)i;
        if (!f.scope) {
            rest.push_back(Item{f.pen, f.ie, src});
            continue;
        }
        any_scope = true;
        if (proto != 9) {
            scope.push_back(Item{f.pen, f.ie, src});
            continue;
        }
        switch (f.ie) {  // normalize.rs:100-135
        case 1: break;   // System: the peer address already identifies the system
        case 2:
            scope.push_back(Item{0, IE_ingressInterface, src});
            scope.push_back(Item{0, IE_egressInterface, src});
            break;
        case 3: scope.push_back(Item{0, IE_lineCardId, src}); break;
        default:  // Cache, Template, Unknown
            out->klass = NGZ_OPTIONS_UNCLASSIFIED;
            out->outcome = NGZ_OPTIONS_OUT_CONVERSION;
            return NGZ_OK;
        }
    }
    if (!any_scope) {  // normalize.rs:60-62, 95-97; the actor filters these out (actor.rs:246, 288)
        out->klass = NGZ_OPTIONS_NONE;
        out->outcome = NGZ_OPTIONS_OUT_NOT_OPTIONS;
        return NGZ_OK;
    }
    auto has = [&](uint16_t ie) { return first_of(scope, ie) || first_of(rest, ie); };  // types.rs:219-221
    auto get = [&](uint16_t ie) {                                                        // types.rs:229-233
        const Item *x = first_of(scope, ie);
        return x ? x : first_of(rest, ie);
    };
    const bool sampling = has(IE_samplingInterval) || has(IE_samplerRandomInterval) ||
                          (has(IE_samplingPacketInterval) && has(IE_samplingPacketSpace)) ||
                          (has(IE_samplingTimeInterval) && has(IE_samplingTimeSpace)) ||
                          (has(IE_samplingSize) && has(IE_samplingPopulation)) || has(IE_samplingProbability);
    const bool iface = (has(IE_ingressInterface) || has(IE_egressInterface)) &&
                       (has(IE_interfaceName) || has(IE_interfaceDescription));
    const bool vrf = (has(IE_ingressVRFID) || has(IE_egressVRFID)) && (has(IE_VRFname) || has(IE_mplsVpnRouteDistinguisher));
    out->klass = sampling ? NGZ_OPTIONS_SAMPLING : iface ? NGZ_OPTIONS_INTERFACE : vrf ? NGZ_OPTIONS_VRF : NGZ_OPTIONS_UNCLASSIFIED;
    out->outcome = NGZ_OPTIONS_OUT_OPS;
    auto is_ie = [](const Item &x, uint16_t ie) { return x.pen == 0 && x.ie == ie; };

    if (out->klass == NGZ_OPTIONS_SAMPLING || out->klass == NGZ_OPTIONS_UNCLASSIFIED) {  // :192-215, 463-483
        Items sc, fl;
        for (const Item &x : scope)
            if (!is_ie(x, IE_paddingOctets) && !is_ie(x, IE_exportingProcessId)) sc.push_back(x);
        for (const Item &x : rest)
            if (!is_ie(x, IE_paddingOctets)) fl.push_back(x);
        if (fl.empty()) return NGZ_OK;  // the upsert has no fields: dropped (handlers.rs:71-74)
        if (emit(sc, out->scope[0], out->scope_src[0], &out->n_scope[0]) ||
            emit(fl, out->fields[0], out->fields_src[0], &out->n_fields[0]))
            return NGZ_E_LIMIT;
        out->n_ops = 1;
        return NGZ_OK;
    }

    // interface (:283-344) and VRF (:407-460) records: one record per direction
    const bool is_if = out->klass == NGZ_OPTIONS_INTERFACE;
    const uint16_t id_ie[2] = {is_if ? IE_ingressInterface : IE_ingressVRFID, is_if ? IE_egressInterface : IE_egressVRFID};
    const uint16_t name_ie[2] = {is_if ? IE_interfaceName : IE_VRFname, is_if ? IE_interfaceDescription : IE_mplsVpnRouteDistinguisher};
    const uint16_t tag[2][2] = {{uint16_t(is_if ? 8 : 12), uint16_t(is_if ? 10 : 14)},   // ingress: name, description / rd
                                {uint16_t(is_if ? 9 : 13), uint16_t(is_if ? 11 : 15)}};  // egress
    const Item *id[2] = {get(id_ie[0]), get(id_ie[1])};
    const Item *name[2] = {first_of(rest, name_ie[0]), first_of(rest, name_ie[1])};  // non-scope fields only
    Items add_scope;
    for (const Item &x : scope)
        if (!is_ie(x, id_ie[0]) && !is_ie(x, id_ie[1]) && !is_ie(x, IE_paddingOctets) && !is_ie(x, IE_exportingProcessId))
            add_scope.push_back(x);
    for (int d = 0; d < 2; ++d)
        if (id[d]) out->id_src[d] = id[d]->src;
    // both directions: their ids must be equal (:307-311); one column read twice always is
    out->id_equal = id[0] && id[1] && id[0]->src != id[1]->src;
    if (!name[0] && !name[1]) {  // every create_*_record returns None (:268-272)
        out->outcome = NGZ_OPTIONS_OUT_MISSING;
        return NGZ_OK;
    }
    for (int d = 0; d < 2; ++d) {
        if (!id[d]) continue;
        Items sc, fl;
        sc.push_back(*id[d]);
        sc.insert(sc.end(), add_scope.begin(), add_scope.end());
        for (int k = 0; k < 2; ++k)
            if (name[k]) fl.push_back(Item{PEN_NETGAUZE, tag[d][k], name[k]->src});
        const int op = out->n_ops++;
        if (emit(sc, out->scope[op], out->scope_src[op], &out->n_scope[op]) ||
            emit(fl, out->fields[op], out->fields_src[op], &out->n_fields[op]))
            return NGZ_E_LIMIT;
    }
    return NGZ_OK;
}

}  // namespace ngzo

extern "C" int ngz_options_template_plan(const uint8_t *tmpl, size_t len, int proto, ngz_options_plan *out) {
    if (!tmpl || !out) return NGZ_E_INVALID;
    memset(out, 0, sizeof *out);
    const bool options = (proto & NGZ_OPTIONS_OPTIONS) != 0;
    proto &= ~NGZ_OPTIONS_OPTIONS;
    if (proto != 10 && proto != 9) return NGZ_E_INVALID;
    std::vector<ngzo::PlanField> fields;
    const int rc = ngzt::walk_template_record(tmpl, len, proto, options, [&](const ngzt::FieldSpec &f) {
        ngzo::PlanField pf;
        pf.pen = f.pen;
        pf.ie = f.ie;
        pf.scope = f.scope;
        fields.push_back(pf);
    });
    if (rc) return rc;
    return ngzo::plan_fields(fields, proto, out);
}
