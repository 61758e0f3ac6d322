// The host side of the flow output (include/ngz/flow_output.h): the validated config
// (FieldConfig::validate and the accepted subset), the schema text (get_avro_schema) and the plan of
// a template's records: everything of crates/collector/src/flow/config.rs:56-763 that the config and
// the template decide.  No HIP: builds with a plain C++17 compiler (tests/native/output_plan_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "ngz/flow_output.h"

namespace ngzout {

// How one source column becomes Avro bytes (host and device)
enum Enc : uint8_t {
    ENC_INT_U = 1,   // unsigned integer column -> long / int (a u64 reads as i64)
    ENC_INT_S,       // signed integer column
    ENC_RAW,         // float32 / float64: the column's bytes
    ENC_BOOL,        // one byte
    ENC_STR,         // string: a fixed column up to its first NUL, or a variable-length cell
    ENC_BYTES,       // bytes: a fixed column, a variable-length cell, or the 32 bytes of an unsigned256
    ENC_MAC,         // "aa:bb:cc:dd:ee:ff"
    ENC_IP4,         // dotted decimal
    ENC_IP6,         // Rust's Ipv6Addr Display
    ENC_DEC_U,       // decimal text of an unsigned integer
    ENC_DEC_S,       // decimal text of a signed integer
    ENC_BOOLSTR,     // "true" / "false"
    ENC_MPLS_ITEM,   // "{n}-{label}" inside an MplsIndex array
    ENC_TS_SECS,     // TimestampMillisString: the decimal text of a dateTime's whole seconds (aggregated
                     // rows only, flow_agg_output.h; its reader hands the seconds on as ENC_DEC_S)
};

struct CfgRef {
    uint32_t pen;
    uint16_t ie, index;
    uint8_t enc;     // Enc
    uint8_t mpls_n;  // ENC_MPLS_ITEM: the n of mplsLabelStackSection{n}
};

struct CfgField {
    std::string name;
    uint8_t select = 0, transform = 0, avro = 0;
    bool nullable = true;
    uint8_t l2_encap = 0;
    uint64_t l2_mask = 0;
    std::vector<CfgRef> refs;
    std::vector<uint8_t> def;  // the default as Avro bytes (a field with a default)
};

struct Config {
    std::vector<CfgField> fields;
};

struct TField {  // one field specifier of a template, scope fields first
    uint32_t pen = 0;
    uint16_t ie = 0;
    bool scope = false;
};

// The zigzag varint of v appended to out
void put_long(std::vector<uint8_t> &out, int64_t v);

// NGZ_OK, or NGZ_OUTPUT_E_UNSUPPORTED / NGZ_OUTPUT_E_CONFIG / NGZ_E_LIMIT / NGZ_E_INVALID with *err
// naming the field.  timestamp_string: TimestampMillisString on the dateTime IEs is accepted (the
// aggregated rows' stage); the column stage refuses it with every other unbuilt transform
int build_config(const ngz_output_field *fields, uint32_t n, Config *cfg, std::string *err, bool timestamp_string = false);

// get_avro_schema's text
std::string schema_text(const Config &cfg);

// The plan of a template's records; NGZ_OK, or NGZ_E_LIMIT past NGZ_OUTPUT_MAX_SOURCES.  Field f's
// present refs are cfg.fields[f].refs[ref_of[f][i]], read from template field plan->f[f].src[i].
int plan_fields(const Config &cfg, const std::vector<TField> &tmpl, ngz_output_plan *plan,
                std::vector<std::vector<uint8_t>> *ref_of);

// ngz_output_template_plan
int template_plan(const Config &cfg, const uint8_t *tmpl, size_t len, int proto, ngz_output_plan *plan);

}  // namespace ngzout
