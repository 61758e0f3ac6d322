"""Python restatement of the reference collector's flow enrichment
(crates/collector/src/flow/enrichment/cache.rs:60-529, actor.rs:122-271).  The checker of
include/ngz/flow_enrich.h.

A field is (pen, ie_id, kind, value bytes) with the value in the canonical column encoding
(DESIGN.md §3), where byte equality is Field equality.  An operation is a dict:
  {"op": "upsert" | "delete" | "delete_all", "ip": str, "domain": int, "weight": int,
   "scope": [field], "fields": [field] (upsert), "ies": [(pen, ie_id)] (delete)}.
"""
K_UINT, K_TCPFLAGS, K_SINT, K_BOOL, K_BYTES, K_U256, K_DTMS, K_DTFRAC, K_STR = range(1, 10)
K_VLEN = 11
STAT_KEYS = ("records_processed", "records_matched", "fields_added", "records_dropped")
WRITER_ID_IE = (3746, 7)  # NetGauze::dataCollectionManifestName


def index_fields(fields):
    """FieldRef (pen, ie_id, occurrence index) of each field of a list (FieldRef::map_fields)."""
    seen, out = {}, []
    for f in fields:
        k = (f[0], f[1])
        out.append((f[0], f[1], seen.get(k, 0)))
        seen[k] = seen.get(k, 0) + 1
    return out


def _value_order(kind, value):
    """Order of two values of one IE: integers by value, anything else bytewise."""
    if kind in (K_UINT, K_BOOL, K_TCPFLAGS):
        return (kind, int.from_bytes(value, "little"), len(value), b"")
    if kind in (K_SINT, K_DTMS):
        return (kind, int.from_bytes(value, "little", signed=True), len(value), b"")
    return (kind, 0, 0, bytes(value))


def scope_order(scope_key):
    """Sort key of a scope in its map: the Rust Ord of Box<[(FieldRef, Field)]> (a prefix first)."""
    # the IE enum declares the vendors' IEs before the IANA ones (generator.rs:1160-1164)
    return tuple(((ref[0] == 0,) + tuple(ref), _value_order(kind, value)) for ref, kind, value in scope_key)


class Cache:
    """EnrichmentCache: ip -> {"global": {scope key: {FieldRef: (weight, kind, value)}},
    "domains": {obs_domain_id: the same}}."""

    def __init__(self):
        self.peers = {}

    @staticmethod
    def scope_key(scope):
        return tuple((ref, f[2], bytes(f[3])) for ref, f in zip(index_fields(scope), scope))

    def apply(self, op):
        """apply_enrichment (cache.rs:96-120)."""
        key = self.scope_key(op["scope"])
        if op["op"] == "upsert":
            self._upsert(op["ip"], op["domain"], key, op["weight"], op["fields"])
        else:
            self._delete(op["ip"], op["domain"], key, op["weight"], None if op["op"] == "delete_all" else op["ies"])

    def _upsert(self, ip, domain, key, weight, fields):  # cache.rs:128-232
        if not fields:
            return
        pm = self.peers.setdefault(ip, {"global": {}, "domains": {}})
        target = pm["global"] if domain == 0 else pm["domains"].setdefault(domain, {})
        md = target.setdefault(key, {})
        for ref, f in zip(index_fields(fields), fields):
            if ref not in md or weight >= md[ref][0]:
                md[ref] = (weight, f[2], bytes(f[3]))

    def _delete(self, ip, domain, key, weight, ies):  # cache.rs:239-325
        if ies is not None and not ies:
            return
        pm = self.peers.get(ip)
        if pm is None:
            return
        if domain == 0:
            target = pm["global"]
        else:
            target = pm["domains"].get(domain)
            if target is None:
                return
        md = target.get(key)
        if md is None:
            return
        listed = None if ies is None else {tuple(x) for x in ies}
        for ref in [r for r, (w, _k, _v) in md.items() if w <= weight and (listed is None or (r[0], r[1]) in listed)]:
            del md[ref]
        if not md:
            del target[key]
            if domain != 0 and not target:
                del pm["domains"][domain]
            if not pm["global"] and not pm["domains"]:
                del self.peers[ip]

    def lookup(self, ip, domain, record, trace=None):
        """get_enrichment_fields (cache.rs:437-528): [(pen, ie_id, index, kind, value, weight)] in
        ascending FieldRef.  `trace`, a dict, receives "max_scopes" (most scopes one record matched) and "ties" (equal-weight
        replacements)."""
        pm = self.peers.get(ip)
        if pm is None:
            return []
        have = {ref: (f[2], bytes(f[3])) for ref, f in zip(index_fields(record), record)}
        best, n_scopes = {}, 0
        maps = [pm["global"]]
        if domain in pm["domains"]:
            maps.append(pm["domains"][domain])
        for m in maps:
            for key in sorted(m, key=scope_order):
                if not all(have.get(ref) == (kind, value) for ref, kind, value in key):
                    continue
                n_scopes += 1
                for ref, wf in m[key].items():
                    if ref in best and wf[0] < best[ref][0]:
                        continue
                    if trace is not None and ref in best and wf[0] == best[ref][0]:
                        trace["ties"] = trace.get("ties", 0) + 1
                    best[ref] = wf
        if trace is not None:
            trace["max_scopes"] = max(trace.get("max_scopes", 0), n_scopes)
        return [(ref[0], ref[1], ref[2], wf[1], wf[2], wf[0]) for ref, wf in sorted(best.items())]


def record_fields(slot, fields):
    """The oracle's non-scope [Field] of a record of `slot` (a product batch slot: its column kinds
    and widths) as restatement fields."""
    import parity
    import ngz_oracle as O
    out = []
    n_scope = sum(1 for fi in slot.fields if fi.is_scope)
    for fi, fv in zip(slot.fields[n_scope:], fields):
        if fi.kind in (K_STR, K_VLEN):
            v = fv.value if isinstance(fv, O.Field) else fv
            value = v.encode("utf-8") if isinstance(v, str) else bytes(v)
        else:
            value = parity.canon(fv, fi)
        out.append((fi.pen, fi.ie_id, fi.kind, value))
    return out


def enrich_batch(cache, ip, batch, oracle, trace=None):
    """EnrichmentActor::enrich (actor.rs:122-271) over every ("ok", packet) of
    parity.oracle_datagrams' list, laid out by the product batch's sets.  Returns (stats,
    {slot: [resolved fields or None per row]}): None for rows of failed messages and of records with
    scope fields, else lookup()'s list."""
    stats = dict.fromkeys(STAT_KEYS, 0)
    rows = {s: [None] * batch.slots[s].n_records for s in range(len(batch.slots))}
    hdr = batch.dgram_headers()
    by_dg = {}
    for gs in batch.sets():
        by_dg.setdefault(int(gs["dgram"]), []).append(gs)
    for d, (kind, pkt) in enumerate(oracle):
        if kind != "ok":
            continue
        data_sets = [s for s in pkt.sets if s[0] == "Data"]
        for (_, _sid, recs), gs in zip(data_sets, by_dg.get(d, [])):
            s, rec0 = int(gs["slot"]), int(gs["rec0"])
            for r, (scope, fields) in enumerate(recs):
                if len(scope):
                    stats["records_dropped"] += 1
                    continue
                stats["records_processed"] += 1
                got = cache.lookup(ip, int(hdr[d]["domain"]), record_fields(batch.slots[s], fields), trace)
                rows[s][rec0 + r] = got
                if got:
                    stats["records_matched"] += 1
                    stats["fields_added"] += len(got)
    return stats, rows


def oracle_field(g):
    """A resolved field (pen, ie_id, index, kind, value, weight) as the oracle's Field (integers,
    strings and octets)."""
    import ngz_oracle as O
    kind, value = g[3], g[4]
    if kind == K_UINT:
        v = int.from_bytes(value, "little")
    elif kind == K_STR:
        v = value.decode("utf-8")
    else:
        v = bytes(value)
    return O.Field(O.REGISTRY.lookup(g[0], g[1]), v)


def packet_json(pkt, rows, writer_id, flags=None):
    """serde JSON text of the enriched FlowInfo (actor.rs:122-271): template sets and records with
    scope fields removed, the resolved fields (rows[(data set index, record index)]) appended in the
    canonical order, dataCollectionManifestName(writer_id) last, then isRenormalized(true) for the
    records in `flags` (renorm_ref's flags of the packet)."""
    import ngz_oracle as O
    writer = O.Field(O.REGISTRY.lookup(*WRITER_ID_IE), writer_id)
    renorm = O.Field(O.REGISTRY.lookup(3746, 16), True)
    sets, si = [], 0
    for kind, sid, recs in pkt.sets:
        if kind != "Data":
            continue
        out = []
        for ri, (scope, fields) in enumerate(recs):
            if len(scope):
                continue
            fj = [O.field_json(x) for x in fields] + [O.field_json(oracle_field(g)) for g in rows.get((si, ri), [])]
            fj.append(O.field_json(writer))
            if flags and flags.get((si, ri)):
                fj.append(O.field_json(renorm))
            out.append({"scope_fields": [], "fields": fj})
        sets.append({"Data": {"id": sid, "records": out}})
        si += 1
    if isinstance(pkt, O.NetFlowV9Packet):
        body = {"NetFlowV9": {"version": 9, "sys_up_time": pkt.sys_up_time, "unix_time": pkt.unix_time.to_json(),
                              "sequence_number": pkt.sequence_number, "source_id": pkt.source_id, "sets": sets}}
    else:
        body = {"IPFIX": {"version": 10, "export_time": pkt.export_time.to_json(),
                          "sequence_number": pkt.sequence_number,
                          "observation_domain_id": pkt.observation_domain_id, "sets": sets}}
    return O.dumps(body)


def batch_json(batch, oracle, rows, writer_id, flags=None):
    """[(dgram, json)] the enriched view must give for every ("ok", packet): `rows` is enrich_batch's."""
    by_dg = {}
    for gs in batch.sets():
        by_dg.setdefault(int(gs["dgram"]), []).append(gs)
    out = []
    for d, (kind, pkt) in enumerate(oracle):
        if kind != "ok":
            continue
        per = {}
        for k, gs in enumerate(by_dg.get(d, [])):
            s, rec0 = int(gs["slot"]), int(gs["rec0"])
            for r in range(int(gs["n"])):
                per[(k, r)] = rows[s][rec0 + r] or []
        out.append((d, packet_json(pkt, per, writer_id, flags[d] if flags else None)))
    return out


# ---------------------------------------------------------------------------------------------
# seeded operation sequences shared by the ABI and the native cache checks
# ---------------------------------------------------------------------------------------------
def _u(ie, v, w):
    return (0, ie, K_UINT, int(v).to_bytes(w, "little"))


def random_sequence(rng, steps=12):
    """A list of steps over a small universe, so scopes collide: an operation dict, or
    {"lookup": (ip, domain, record)}."""
    ips = ["10.0.0.1", "2001:db8::1"]
    scopes = [[], [_u(302, 1, 8)], [_u(302, 2, 8)], [_u(10, 5, 4)], [_u(10, 5, 4), _u(14, 6, 4)], [_u(10, 5, 4), _u(10, 7, 4)],
              [(0, 27, K_BYTES, bytes(range(16)))], [(0, 56, K_BYTES, b"\1\2\3\4\5\6")]]
    adds = [_u(34, 100, 4), _u(34, 10, 4), _u(35, 1, 1), (0, 82, K_STR, b"eth0"), (0, 82, K_STR, b""),
            (0, 84, K_STR, b"s" * 300), (0, 95, K_BYTES, b"\xf4"), _u(138, 9, 8)]
    records = [[_u(1, 1500, 8)], [_u(302, 1, 8), _u(10, 5, 4), _u(14, 6, 4)], [_u(10, 5, 4), _u(10, 7, 4), _u(302, 2, 8)],
               [(0, 27, K_BYTES, bytes(range(16))), (0, 56, K_BYTES, b"\1\2\3\4\5\6"), _u(10, 5, 4)], []]
    out = []
    for _ in range(steps):
        x = rng.random()
        ip, dom = rng.choice(ips), rng.choice([0, 0, 1000, 2000])
        w = rng.choice([16, 64, 64, 200])
        if x < 0.45:
            out.append({"op": "upsert", "ip": ip, "domain": dom, "weight": w, "scope": rng.choice(scopes),
                        "fields": [rng.choice(adds) for _ in range(rng.randrange(0, 4))]})
        elif x < 0.6:
            out.append({"op": "delete", "ip": ip, "domain": dom, "weight": w, "scope": rng.choice(scopes),
                        "ies": [rng.choice([(0, 34), (0, 82), (0, 84), (0, 35)]) for _ in range(rng.randrange(0, 3))]})
        elif x < 0.68:
            out.append({"op": "delete_all", "ip": ip, "domain": dom, "weight": w, "scope": rng.choice(scopes)})
        else:
            out.append({"lookup": (ip, rng.choice([1000, 2000, 3000]), rng.choice(records))})
    return out
