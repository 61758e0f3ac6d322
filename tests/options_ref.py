"""Python restatement of the reference collector's flow-options input
(crates/collector/src/inputs/flow_options/normalize.rs:56-496, handlers.rs:53-95, actor.rs:217-326,
over flow/types.rs:138-234).  The checker of include/ngz/flow_options.h.

A field is (pen, ie_id, kind, value bytes) as in enrich_ref.  Where the reference iterates an
FxHashMap (unspecified order) this restatement keeps the record's own order, as the header states.
"""
import enrich_ref as E

STAT_KEYS = ("received_flows", "processed_options_records", "operations_generated", "normalization_errors",
             "netflow_v9_conversion_errors", "ops_refused")
PEN_NETGAUZE = 3746
INGRESS_IF, EGRESS_IF, IF_NAME, IF_DESC = 10, 14, 82, 83
INGRESS_VRF, EGRESS_VRF, VRF_NAME, MPLS_RD = 234, 235, 236, 90
LINE_CARD_ID, EXPORTING_PROCESS_ID, PADDING = 141, 144, 210
# re-tagged NetGauze IEs: (ingress, egress)
TAGS = {IF_NAME: (8, 9), IF_DESC: (10, 11), VRF_NAME: (12, 13), MPLS_RD: (14, 15)}


class NoScopeFields(Exception):
    """OptionsDataRecordError::NoScopeFields (normalize.rs:60-62, 95-97)."""


class ConversionError(Exception):
    """OptionsDataRecordError::UnsupportedNetFlowV9ScopeFieldType (normalize.rs:119-133)."""

    def __init__(self, scope_field):
        super().__init__(scope_field)
        self.scope_field = scope_field


class NormalizationError(Exception):
    """UnsupportedInterfaceType / UnsupportedVrfType / MissingRequiredFields (normalize.rs:32-37)."""

    def __init__(self, kind):
        super().__init__(kind)
        self.kind = kind


def _is(f, ie):
    return f[0] == 0 and f[1] == ie


def _first(fields, ie):
    """FieldRefLookup::get_by_ie of one map (types.rs:164-174): index 0 is the first occurrence."""
    for f in fields:
        if _is(f, ie):
            return f
    return None


def convert_nf9_scope(scope):
    """normalize.rs:99-135: [(scope code, u32 value or bytes[, pen])] -> IPFIX-style scope fields."""
    out = []
    for code, value, *pen in scope:
        pen = pen[0] if pen else 0
        if pen == 0 and code == 1:  # System: ignored
            continue
        if pen == 0 and code == 2:  # Interface -> ingressInterface and egressInterface
            v = int(value).to_bytes(4, "little")
            out += [(0, INGRESS_IF, E.K_UINT, v), (0, EGRESS_IF, E.K_UINT, v)]
        elif pen == 0 and code == 3:  # LineCard -> lineCardId
            out.append((0, LINE_CARD_ID, E.K_UINT, int(value).to_bytes(4, "little")))
        elif pen == 0 and code in (4, 5):
            raise ConversionError("Cache" if code == 4 else "Template")
        else:
            raise ConversionError("Unknown (pen=%d, id=%d)" % (pen, code))
    return out


def _has(scope, fields, ie):
    """IndexedDataRecord::contains_ie (types.rs:219-221): the scope, then the fields."""
    return _first(scope, ie) is not None or _first(fields, ie) is not None


def is_sampling_type(scope, fields):  # normalize.rs:172-189
    has = lambda ie: _has(scope, fields, ie)  # noqa: E731
    return has(34) or has(50) or (has(305) and has(306)) or (has(307) and has(308)) or (has(309) and has(310)) or has(311)


def is_interface_type(scope, fields):  # normalize.rs:218-226
    has = lambda ie: _has(scope, fields, ie)  # noqa: E731
    return (has(INGRESS_IF) or has(EGRESS_IF)) and (has(IF_NAME) or has(IF_DESC))


def is_vrf_type(scope, fields):  # normalize.rs:347-354
    has = lambda ie: _has(scope, fields, ie)  # noqa: E731
    return (has(INGRESS_VRF) or has(EGRESS_VRF)) and (has(VRF_NAME) or has(MPLS_RD))


def classify(scope, fields):
    """normalize.rs:156-169."""
    if is_sampling_type(scope, fields):
        return "sampling"
    if is_interface_type(scope, fields):
        return "interface"
    if is_vrf_type(scope, fields):
        return "vrf"
    return "unclassified"


def try_from(scope, fields, netflow=False):
    """TryFrom<ipfix::DataRecord> (:56-67) / TryFrom<netflow::DataRecord> (:91-141): (class, scope
    fields, fields).  A NetFlow v9 scope is [(code, value[, pen])]."""
    if not scope:
        raise NoScopeFields()
    if netflow:
        scope = convert_nf9_scope(scope)
    return classify(scope, fields), list(scope), list(fields)


def _split(scope, fields, in_ie, out_ie, name_ie, desc_ie, what, check_ids=True):
    """normalize_interface_type (:283-344) / normalize_vrf_type (:407-460)."""
    def get(ie):  # types.rs:229-233: scope first
        f = _first(scope, ie)
        return f if f is not None else _first(fields, ie)

    ids = (get(in_ie), get(out_ie))
    names = [(ie, _first(fields, ie)) for ie in (name_ie, desc_ie)]  # the non-scope fields only (:288-289)
    add_scope = [f for f in scope if not (_is(f, in_ie) or _is(f, out_ie) or _is(f, PADDING) or _is(f, EXPORTING_PROCESS_ID))]
    if check_ids and ids[0] is not None and ids[1] is not None and (ids[0][2], ids[0][3]) != (ids[1][2], ids[1][3]):
        raise NormalizationError("Unsupported%sType" % what)
    records = []
    for d, idf in enumerate(ids):
        if idf is None:
            continue
        out = [(PEN_NETGAUZE, TAGS[ie][d], f[2], f[3]) for ie, f in names if f is not None]
        if out:  # create_*_record returns None without fields (:268-272)
            records.append(([idf] + add_scope, out))
    if not records:
        raise NormalizationError("MissingRequiredFields")
    return records


def normalize_interface_type(scope, fields, check_ids=True):  # normalize.rs:283-344
    return _split(scope, fields, INGRESS_IF, EGRESS_IF, IF_NAME, IF_DESC, "Interface", check_ids)


def normalize_vrf_type(scope, fields, check_ids=True):  # normalize.rs:407-460
    return _split(scope, fields, INGRESS_VRF, EGRESS_VRF, VRF_NAME, MPLS_RD, "Vrf", check_ids)


def normalize_sampling_type(scope, fields):
    """normalize_sampling_type (:192-215); normalize_unclassified_type (:463-483) filters the same."""
    sc = [f for f in scope if not (_is(f, PADDING) or _is(f, EXPORTING_PROCESS_ID))]
    fl = [f for f in fields if not _is(f, PADDING)]
    return [(sc, fl)]


def normalize(scope, fields, check_ids=True):
    """classify + into_normalized_records (:486-495): (class, [(scope fields, fields)])."""
    klass = classify(scope, fields)
    if klass == "interface":
        return klass, normalize_interface_type(scope, fields, check_ids)
    if klass == "vrf":
        return klass, normalize_vrf_type(scope, fields, check_ids)
    return klass, normalize_sampling_type(scope, fields)


def handle(scope, fields, ip, domain, weight):
    """handle_option_record (handlers.rs:53-76): the upserts of one classified record."""
    _klass, records = normalize(scope, fields)
    ops = [{"op": "upsert", "ip": ip, "domain": domain, "weight": weight, "scope": sc, "fields": fl} for sc, fl in records]
    return [op for op in ops if op["fields"]]  # validate(): drop useless no-field ops


def plan(scope_ies, field_ies, proto=10):
    """What the template alone decides, in ngz_options_template_plan's terms: scope_ies / field_ies are
    [(pen, ie_id)] (NetFlow v9 scope: (0, code)).  Every field gets a distinct value, so the id
    equality shows as `id_equal`; the operations' references carry occurrence indices."""
    if not scope_ies:
        return {"class": "none", "outcome": "not_options", "id_equal": False, "ops": []}
    val = lambda i: int(i + 1).to_bytes(4, "little")  # noqa: E731
    n = len(scope_ies)
    if proto == 9:
        try:
            scope = []
            for i, (_pen, code) in enumerate(scope_ies):
                scope += [f[:3] + (val(i),) for f in convert_nf9_scope([(code, i + 1)])]
        except ConversionError:
            return {"class": "unclassified", "outcome": "conversion_error", "id_equal": False, "ops": []}
    else:
        scope = [(pen, ie, E.K_UINT, val(i)) for i, (pen, ie) in enumerate(scope_ies)]
    fields = [(pen, ie, E.K_UINT, val(n + i)) for i, (pen, ie) in enumerate(field_ies)]
    klass = classify(scope, fields)
    src = lambda f: int.from_bytes(f[3], "little") - 1  # noqa: E731
    refs = lambda fl: [r for r in E.index_fields(fl)]  # noqa: E731
    id_equal = False
    if klass in ("interface", "vrf"):  # both directions, read from two different template fields
        ids = (INGRESS_IF, EGRESS_IF) if klass == "interface" else (INGRESS_VRF, EGRESS_VRF)
        got = [_first(scope, ie) or _first(fields, ie) for ie in ids]
        id_equal = got[0] is not None and got[1] is not None and got[0][3] != got[1][3]
    try:
        _k, records = normalize(scope, fields, check_ids=False)
    except NormalizationError:
        return {"class": klass, "outcome": "missing_required_fields", "id_equal": id_equal, "ops": []}
    ops = [{"scope": refs(sc), "fields": refs(fl), "scope_src": [src(f) for f in sc], "fields_src": [src(f) for f in fl]}
           for sc, fl in records if fl]
    return {"class": klass, "outcome": "ops", "id_equal": id_equal, "ops": ops}


def _value(fi, fv):
    """(kind, canonical bytes) of the oracle's value of a field decoded into the column `fi`."""
    import parity
    import ngz_oracle as O
    v = fv.value if isinstance(fv, (O.Field, O.ScopeFieldValue)) else fv
    if fi.kind in (E.K_STR, E.K_VLEN):
        if isinstance(v, str):
            return E.K_STR, v.encode("utf-8")
        return E.K_BYTES, bytes(v)
    if fi.kind == 10:  # NGZ_K_SCOPE32
        return E.K_UINT, int(v).to_bytes(4, "little")
    return fi.kind, parity.canon(fv, fi)


def record_parts(slot, scope, fields, netflow):
    """The oracle's record of `slot` (a product batch slot: its column kinds and widths) as the
    restatement's scope fields and fields; raises ConversionError (NetFlow v9)."""
    n_scope = len(scope)
    fl = [(fi.pen, fi.ie_id) + _value(fi, fv) for fi, fv in zip(slot.fields[n_scope:], fields)]
    if netflow:
        sc = convert_nf9_scope([(fv.ie.id, fv.value, fv.ie.pen) for fv in scope])
    else:
        sc = [(fi.pen, fi.ie_id) + _value(fi, fv) for fi, fv in zip(slot.fields[:n_scope], scope)]
    return sc, fl


def harvest_batch(batch, oracle, ip, weight):
    """FlowOptionsActor::run's flow branch (actor.rs:217-326) over every ("ok", packet) of
    parity.oracle_datagrams' list, laid out by the product batch's sets: (stats, [operation])."""
    import ngz_oracle as O
    stats = dict.fromkeys(STAT_KEYS, 0)
    ops = []
    by_dg = {}
    for gs in batch.sets():
        by_dg.setdefault(int(gs["dgram"]), []).append(gs)
    for d, (kind, pkt) in enumerate(oracle):
        if kind != "ok":
            continue
        stats["received_flows"] += 1
        netflow = isinstance(pkt, O.NetFlowV9Packet)
        domain = pkt.source_id if netflow else pkt.observation_domain_id
        data_sets = [s for s in pkt.sets if s[0] == "Data"]
        for (_, _sid, recs), gs in zip(data_sets, by_dg.get(d, [])):
            slot = batch.slots[int(gs["slot"])]
            for scope, fields in recs:
                if not len(scope):
                    continue
                stats["processed_options_records"] += 1
                try:
                    sc, fl = record_parts(slot, scope, fields, netflow)
                except ConversionError:
                    stats["netflow_v9_conversion_errors"] += 1
                    continue
                try:
                    got = handle(sc, fl, ip, domain, weight)
                except NormalizationError:
                    stats["normalization_errors"] += 1
                    continue
                stats["operations_generated"] += len(got)
                ops += got
    return stats, ops
