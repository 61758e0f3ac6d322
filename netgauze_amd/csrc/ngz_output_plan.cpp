// The host side of the flow output: see ngz_output_plan.h.  No HIP.
#include "ngz_output_plan.h"

#include <cstring>
#include <map>
#include <set>

#include "ngz_template_record.h"

namespace ngzout {
namespace {

// IE registry rows (generated from the reference XML, tools/gen_ie_registry.py); this unit keeps its
// own copy of the table so that it builds without the decode sources
struct IeRow {
    uint32_t pen;
    uint16_t id;
    uint8_t dtype;  // RFC 7012 order, NGZ_DT_*
    uint8_t flags;  // 1 MPLS label, 2 tcpControlBits, 4 sub-registry
};
#define NGZ_IE(pen, id, dt, fl, nm) {pen, (uint16_t)(id), (uint8_t)(dt), (uint8_t)(fl)},
#define NGZ_VENDOR(pen, nm)
const IeRow kIes[] = {
#include "ie_table.inc"
};
#undef NGZ_IE
#undef NGZ_VENDOR

const IeRow *ie_find(uint32_t pen, uint16_t id) {
    static const std::map<uint64_t, const IeRow *> index = [] {
        std::map<uint64_t, const IeRow *> m;
        for (const IeRow &r : kIes) m[((uint64_t)r.pen << 16) | r.id] = &r;
        return m;
    }();
    auto it = index.find(((uint64_t)pen << 16) | id);
    return it == index.end() ? nullptr : it->second;
}

constexpr uint8_t T_TS_MILLIS = 9, T_TS_MICROS = 10, T_TS_NANOS = 11;  // avro kinds no accepted field has

// ie_avro_type (config.rs:766-793)
uint8_t ie_avro_type(const IeRow &r) {
    switch (r.dtype) {
    case NGZ_DT_UNSIGNED8: case NGZ_DT_UNSIGNED16: case NGZ_DT_SIGNED8: case NGZ_DT_SIGNED16: case NGZ_DT_SIGNED32:
        return NGZ_OUT_T_INT;
    case NGZ_DT_UNSIGNED32: case NGZ_DT_UNSIGNED64: case NGZ_DT_SIGNED64: return NGZ_OUT_T_LONG;
    case NGZ_DT_FLOAT32: return NGZ_OUT_T_FLOAT;
    case NGZ_DT_FLOAT64: return NGZ_OUT_T_DOUBLE;
    case NGZ_DT_BOOLEAN: return NGZ_OUT_T_BOOLEAN;
    case NGZ_DT_MAC_ADDRESS: case NGZ_DT_STRING: case NGZ_DT_IPV4_ADDRESS: case NGZ_DT_IPV6_ADDRESS: return NGZ_OUT_T_STRING;
    case NGZ_DT_DATETIME_SECONDS: case NGZ_DT_DATETIME_MILLISECONDS: return T_TS_MILLIS;
    case NGZ_DT_DATETIME_MICROSECONDS: return T_TS_MICROS;
    case NGZ_DT_DATETIME_NANOSECONDS: return T_TS_NANOS;
    default: return NGZ_OUT_T_BYTES;
    }
}

bool is_datetime(const IeRow &r) { return r.dtype >= NGZ_DT_DATETIME_SECONDS && r.dtype <= NGZ_DT_DATETIME_NANOSECONDS; }

// n of mplsLabelStackSection{n} (config.rs:395-413, 981-992), or 0
uint8_t mpls_index_n(uint32_t pen, uint16_t ie) {
    if (pen) return 0;
    if (ie == 316) return 1;
    return ie >= 71 && ie <= 79 ? (uint8_t)(ie - 69) : 0;
}

const char *avro_name(uint8_t t) {
    static const char *n[] = {"", "int", "long", "float", "double", "boolean", "string", "bytes", "array"};
    return n[t];
}

// RawValue::avro_type of a default (flow/mod.rs:57-76), or 0
uint8_t default_avro_type(uint8_t kind) {
    switch (kind) {
    case NGZ_OUT_DEF_BYTES: return NGZ_OUT_T_BYTES;
    case NGZ_OUT_DEF_U8: case NGZ_OUT_DEF_U16: case NGZ_OUT_DEF_I8: case NGZ_OUT_DEF_I16: case NGZ_OUT_DEF_I32: return NGZ_OUT_T_INT;
    case NGZ_OUT_DEF_U32: case NGZ_OUT_DEF_U64: case NGZ_OUT_DEF_I64: return NGZ_OUT_T_LONG;
    case NGZ_OUT_DEF_F32: return NGZ_OUT_T_FLOAT;
    case NGZ_OUT_DEF_F64: return NGZ_OUT_T_DOUBLE;
    case NGZ_OUT_DEF_BOOLEAN: return NGZ_OUT_T_BOOLEAN;
    case NGZ_OUT_DEF_STRING: return NGZ_OUT_T_STRING;
    }
    return 0;
}

struct Refusal {
    int rc;
    std::string why;
};

// The encoding of one ref under Identity or String, or why it is refused
Refusal ref_encoding(const IeRow &r, uint8_t transform, uint8_t *enc) {
    const bool subreg = r.flags & 4, tcp = r.flags & 2, mpls = r.flags & 1;
    const uint8_t t = ie_avro_type(r);
    if (transform == NGZ_OUT_TR_IDENTITY) {
        if (subreg || tcp || mpls || is_datetime(r))
            return {NGZ_OUTPUT_E_UNSUPPORTED, "Identity on an IE whose RawValue is the String fallback (sub-registry, tcpControlBits, MPLS label, dateTime)"};
        switch (r.dtype) {
        case NGZ_DT_UNSIGNED8: case NGZ_DT_UNSIGNED16: case NGZ_DT_UNSIGNED32: case NGZ_DT_UNSIGNED64: *enc = ENC_INT_U; break;
        case NGZ_DT_SIGNED8: case NGZ_DT_SIGNED16: case NGZ_DT_SIGNED32: case NGZ_DT_SIGNED64: *enc = ENC_INT_S; break;
        case NGZ_DT_FLOAT32: case NGZ_DT_FLOAT64: *enc = ENC_RAW; break;
        case NGZ_DT_BOOLEAN: *enc = ENC_BOOL; break;
        case NGZ_DT_MAC_ADDRESS: *enc = ENC_MAC; break;
        case NGZ_DT_STRING: *enc = ENC_STR; break;
        case NGZ_DT_IPV4_ADDRESS: *enc = ENC_IP4; break;
        case NGZ_DT_IPV6_ADDRESS: *enc = ENC_IP6; break;
        default: *enc = ENC_BYTES; break;
        }
        return {NGZ_OK, ""};
    }
    // String: validate_ie_compatibility first (config.rs:419-433)
    if (t == NGZ_OUT_T_BYTES && !(r.pen == 0 && r.id == 90))
        return {NGZ_OUTPUT_E_CONFIG, "String requires String conversion, but the IE is Bytes type"};
    if (subreg || tcp || is_datetime(r) || r.dtype == NGZ_DT_FLOAT32 || r.dtype == NGZ_DT_FLOAT64 || t == NGZ_OUT_T_BYTES)
        return {NGZ_OUTPUT_E_UNSUPPORTED, "String on an IE whose Display text is not pinned (float, dateTime, sub-registry, tcpControlBits, route distinguisher)"};
    switch (r.dtype) {
    case NGZ_DT_UNSIGNED8: case NGZ_DT_UNSIGNED16: case NGZ_DT_UNSIGNED32: case NGZ_DT_UNSIGNED64: *enc = ENC_DEC_U; break;
    case NGZ_DT_SIGNED8: case NGZ_DT_SIGNED16: case NGZ_DT_SIGNED32: case NGZ_DT_SIGNED64: *enc = ENC_DEC_S; break;
    case NGZ_DT_BOOLEAN: *enc = ENC_BOOLSTR; break;
    case NGZ_DT_MAC_ADDRESS: *enc = ENC_MAC; break;
    case NGZ_DT_STRING: *enc = ENC_STR; break;
    case NGZ_DT_IPV4_ADDRESS: *enc = ENC_IP4; break;
    default: *enc = ENC_IP6; break;
    }
    return {NGZ_OK, ""};
}

Refusal build_field(const ngz_output_field &in, CfgField *f, bool timestamp_string) {
    if (!in.name || !in.name[0]) return {NGZ_E_INVALID, "a field without a name"};
    f->name = in.name;
    if (f->name.size() > NGZ_OUTPUT_MAX_NAME) return {NGZ_E_LIMIT, "a name longer than 128 bytes"};
    if (f->name.find("custom_primitives.") != std::string::npos)
        return {NGZ_OUTPUT_E_UNSUPPORTED, "custom_primitives fields (a map) are not built"};
    if (in.select > NGZ_OUT_SEL_L2SEGMENT || in.transform > NGZ_OUT_TR_STRING_MAP_AGG || in.default_kind > NGZ_OUT_DEF_STRING_MAP)
        return {NGZ_E_INVALID, "an unknown select, transform or default kind"};
    if (in.n_refs && !in.refs) return {NGZ_E_INVALID, "refs is null"};
    f->select = in.select;
    f->transform = in.transform;
    // validate (config.rs:254-281): the select's IEs
    if (!in.n_refs) {
        if (in.select == NGZ_OUT_SEL_COALESCE) return {NGZ_OUTPUT_E_CONFIG, "Coalesce list cannot be empty"};
        if (in.select == NGZ_OUT_SEL_MULTI) return {NGZ_OUTPUT_E_CONFIG, "Multi-select list cannot be empty"};
        return {NGZ_E_INVALID, "a select without an IE"};
    }
    if ((in.select == NGZ_OUT_SEL_SINGLE || in.select == NGZ_OUT_SEL_L2SEGMENT) && in.n_refs != 1)
        return {NGZ_E_INVALID, "Single and Layer2SegmentId select one IE"};
    const bool ts = timestamp_string && in.transform == NGZ_OUT_TR_TIMESTAMP_MILLIS_STRING;
    if (in.transform > NGZ_OUT_TR_MPLS_INDEX && !ts)
        return {NGZ_OUTPUT_E_UNSUPPORTED, "only the Identity, String and MplsIndex transforms are built"};
    // validate_select_transform_compatibility (:283-367)
    const bool multi = in.select == NGZ_OUT_SEL_MULTI, agg = in.transform == NGZ_OUT_TR_MPLS_INDEX;
    if (multi && !agg) return {NGZ_OUTPUT_E_CONFIG, "Multi selection requires an aggregating transform"};
    if (!multi && agg) return {NGZ_OUTPUT_E_CONFIG, "MplsIndex requires Multi selection"};
    if (in.n_refs > (multi ? NGZ_OUTPUT_MAX_REFS : NGZ_OUTPUT_MAX_COALESCE)) return {NGZ_E_LIMIT, "more refs than a select may hold (8, Multi 10)"};
    std::vector<const IeRow *> rows;
    for (uint32_t i = 0; i < in.n_refs; ++i) {
        const IeRow *r = ie_find(in.refs[i].pen, in.refs[i].ie_id);
        if (!r) return {NGZ_OUTPUT_E_UNSUPPORTED, "an IE the registry does not know"};
        rows.push_back(r);
    }
    if (in.select == NGZ_OUT_SEL_COALESCE && in.transform == NGZ_OUT_TR_IDENTITY)
        for (const IeRow *r : rows)
            if (ie_avro_type(*r) != ie_avro_type(*rows[0]))
                return {NGZ_OUTPUT_E_CONFIG, "Coalesce selection with mixed types requires an explicit transform"};
    if (in.select == NGZ_OUT_SEL_L2SEGMENT && !(rows[0]->pen == 0 && rows[0]->id == 351))
        return {NGZ_OUTPUT_E_CONFIG, "Layer2SegmentId requires layer2SegmentId IE"};
    // validate_ie_compatibility (:369-439) and the accepted subset, per IE
    for (uint32_t i = 0; i < in.n_refs; ++i) {
        CfgRef ref{in.refs[i].pen, in.refs[i].ie_id, in.refs[i].index, 0, 0};
        if (agg) {
            ref.mpls_n = mpls_index_n(ref.pen, ref.ie);
            ref.enc = ENC_MPLS_ITEM;
            if (!ref.mpls_n) return {NGZ_OUTPUT_E_CONFIG, "MplsIndex requires MPLS label stack fields"};
        } else if (ts) {  // validate_ie_compatibility (:371-385); then ts.timestamp().to_string() (:934-940)
            if (!is_datetime(*rows[i])) return {NGZ_OUTPUT_E_CONFIG, "TimestampMillisString requires timestamp IE"};
            ref.enc = ENC_TS_SECS;
        } else {
            const Refusal r = ref_encoding(*rows[i], in.transform, &ref.enc);
            if (r.rc) return r;
        }
        f->refs.push_back(ref);
    }
    // avro_type (:528-530)
    if (agg) f->avro = NGZ_OUT_T_ARRAY;
    else if (in.transform == NGZ_OUT_TR_STRING || ts) f->avro = NGZ_OUT_T_STRING;
    else if (in.select == NGZ_OUT_SEL_L2SEGMENT) f->avro = NGZ_OUT_T_LONG;
    else f->avro = ie_avro_type(*rows[0]);
    if (in.select == NGZ_OUT_SEL_L2SEGMENT) {
        f->l2_encap = in.encap_type;
        f->l2_mask = !in.encap_unassigned && (in.encap_type == 1 || in.encap_type == 2) ? 0xFFFFFFull : 0xFFFFFFFFFFull;
    }
    // validate_default (:441-452) and its Avro bytes
    f->nullable = in.default_kind == NGZ_OUT_DEF_NONE;
    if (!f->nullable) {
        const uint8_t dt = default_avro_type(in.default_kind);
        if (!dt) return {NGZ_OUTPUT_E_UNSUPPORTED, "only scalar, string and bytes defaults are built"};
        if (dt != f->avro) return {NGZ_OUTPUT_E_CONFIG, std::string("Default type mismatch: expected ") + avro_name(f->avro) + ", " + avro_name(dt)};
        const uint64_t v = in.default_scalar;
        switch (in.default_kind) {
        case NGZ_OUT_DEF_U8: put_long(f->def, (int64_t)(v & 0xFF)); break;
        case NGZ_OUT_DEF_U16: put_long(f->def, (int64_t)(v & 0xFFFF)); break;
        case NGZ_OUT_DEF_U32: put_long(f->def, (int64_t)(v & 0xFFFFFFFFull)); break;
        case NGZ_OUT_DEF_I8: put_long(f->def, (int8_t)v); break;
        case NGZ_OUT_DEF_I16: put_long(f->def, (int16_t)v); break;
        case NGZ_OUT_DEF_I32: put_long(f->def, (int32_t)v); break;
        case NGZ_OUT_DEF_U64: case NGZ_OUT_DEF_I64: put_long(f->def, (int64_t)v); break;
        case NGZ_OUT_DEF_F32: for (int b = 0; b < 4; ++b) f->def.push_back((uint8_t)(v >> (8 * b))); break;
        case NGZ_OUT_DEF_F64: for (int b = 0; b < 8; ++b) f->def.push_back((uint8_t)(v >> (8 * b))); break;
        case NGZ_OUT_DEF_BOOLEAN: f->def.push_back(v ? 1 : 0); break;
        default:
            if (in.default_len && !in.default_bytes) return {NGZ_E_INVALID, "default_bytes is null"};
            put_long(f->def, in.default_len);
            f->def.insert(f->def.end(), in.default_bytes, in.default_bytes + in.default_len);
        }
        if (f->def.size() > NGZ_OUTPUT_MAX_DEFAULT) return {NGZ_E_LIMIT, "a default longer than 64 encoded bytes"};
    }
    return {NGZ_OK, ""};
}

}  // namespace

void put_long(std::vector<uint8_t> &out, int64_t v) {
    uint64_t z = ((uint64_t)v << 1) ^ (uint64_t)(v >> 63);
    while (z >= 0x80) {
        out.push_back((uint8_t)(z | 0x80));
        z >>= 7;
    }
    out.push_back((uint8_t)z);
}

int build_config(const ngz_output_field *fields, uint32_t n, Config *cfg, std::string *err, bool timestamp_string) {
    cfg->fields.clear();
    if (n && !fields) return NGZ_E_INVALID;
    if (n > NGZ_OUTPUT_MAX_FIELDS) {
        *err = "more than 64 output fields";
        return NGZ_E_LIMIT;
    }
    std::set<std::string> names;
    for (uint32_t i = 0; i < n; ++i) {
        CfgField f;
        Refusal r = build_field(fields[i], &f, timestamp_string);
        if (!r.rc && !names.insert(f.name).second) r = {NGZ_E_INVALID, "a field name given twice"};
        if (r.rc) {
            *err = "Invalid FieldConfig for " + (fields[i].name ? std::string(fields[i].name) : "field " + std::to_string(i)) +
                   ", reason: " + r.why;
            return r.rc;
        }
        cfg->fields.push_back(std::move(f));
    }
    return NGZ_OK;
}

std::string schema_text(const Config &cfg) {
    std::string s = "{\n  \"type\": \"record\",\n  \"name\": \"acct_data\",\n  \"fields\": [\n";
    for (size_t i = 0; i < cfg.fields.size(); ++i) {
        const CfgField &f = cfg.fields[i];
        std::string t = f.avro == NGZ_OUT_T_ARRAY ? "{\"type\": \"array\", \"items\": \"string\"}"
                                                  : std::string("\"") + avro_name(f.avro) + "\"";
        if (f.nullable) t = "[\"null\", " + t + "]";
        s += "    { \"name\": \"" + f.name + "\", \"type\": " + t + " }";
        s += i + 1 < cfg.fields.size() ? ",\n" : "";
    }
    return s + "\n  ]\n}";
}

int plan_fields(const Config &cfg, const std::vector<TField> &tmpl, ngz_output_plan *plan, std::vector<std::vector<uint8_t>> *ref_of) {
    memset(plan, 0, sizeof *plan);
    plan->n_fields = (uint32_t)cfg.fields.size();
    if (ref_of) ref_of->assign(cfg.fields.size(), {});
    // FieldRef -> template field, occurrences counted over the non-scope fields (config.rs:194-213)
    std::map<uint64_t, uint32_t> seen;
    std::map<std::pair<uint64_t, uint32_t>, int16_t> at;
    for (size_t i = 0; i < tmpl.size() && i < 0x7FFF; ++i) {
        if (tmpl[i].scope) continue;
        const uint64_t key = ((uint64_t)tmpl[i].pen << 16) | tmpl[i].ie;
        at[{key, seen[key]++}] = (int16_t)i;
    }
    uint32_t n_sources = 0;
    for (size_t fi = 0; fi < cfg.fields.size(); ++fi) {
        const CfgField &f = cfg.fields[fi];
        ngz_output_field_plan &p = plan->f[fi];
        p.avro_type = f.avro;
        p.nullable = f.nullable;
        for (int16_t &s : p.src) s = -1;
        for (size_t i = 0; i < f.refs.size(); ++i) {
            auto it = at.find({((uint64_t)f.refs[i].pen << 16) | f.refs[i].ie, f.refs[i].index});
            if (it == at.end()) continue;
            p.src[p.n_present++] = it->second;
            if (ref_of) (*ref_of)[fi].push_back((uint8_t)i);
            if (f.select != NGZ_OUT_SEL_MULTI) break;  // Coalesce: the first one present
        }
        n_sources += p.n_present;
    }
    return n_sources > NGZ_OUTPUT_MAX_SOURCES ? NGZ_E_LIMIT : NGZ_OK;
}

int template_plan(const Config &cfg, const uint8_t *tmpl, size_t len, int proto, ngz_output_plan *plan) {
    const bool options = (proto & NGZ_OUTPUT_OPTIONS) != 0;
    proto &= ~NGZ_OUTPUT_OPTIONS;
    if (!tmpl || !plan || (proto != 10 && proto != 9)) return NGZ_E_INVALID;
    std::vector<TField> fields;
    const int rc = ngzt::walk_template_record(tmpl, len, proto, options,
                                              [&](const ngzt::FieldSpec &f) { fields.push_back(TField{f.pen, f.ie, f.scope}); });
    if (rc) return rc;
    return plan_fields(cfg, fields, plan, nullptr);
}

}  // namespace ngzout
