// qe_pernode.cpp -- QE_EXEC_PER_NODE: the kernel-per-expression-node pipeline on one HIP stream.
//
// The on-device analogue of Mode.INTERPRETER's tree walk (evaluator/Interpreter.kt:29-109): every
// node of the typed tree becomes one launch of a precompiled kernel (qe_pernode_kernels.hip) over
// whole columns; BOOLEAN values and validity travel as 64-row bitmap words.  The executor is
// filter-first, conjunct by conjunct (late materialisation at node granularity):
//   1. the Filter's top-level AND chain is split into its conjuncts (split_conjuncts; the reference's AND is lazy in the same
//      direction, Interpreter.kt:54-72)
//   2. a conjunct is evaluated over the CURRENT domain -> keep = value & known -> word popcounts -> scan; when at most half
//      of the domain survives (or it is the last conjunct) the domain is narrowed to the kept rows: ascending row ids,
//      columns already gathered are re-gathered from their compact copies
//   3. a column is gathered from the batch only when a node first needs it in a narrowed domain -- at that domain's
//      density: cfg 2 reads `a` in full, `c` where a < 100 and `b` (and `a` again) only for the rows finally kept
//   4. the Projection's nodes are evaluated over the final domain
// It needs no JIT and is the general path; the fused kernel (qe_codegen.cpp) is the fast path.
#include "qe_pernode.h"

#include <cstdlib>
#include <algorithm>

#include "qe_exec.h"
#include "qe_expr_rules.h"
#include "qe_kernels.h"
#include "qe_pernode_kernels.h"
#include "qe_scan.h"

namespace qe {

namespace {

using Buf = std::shared_ptr<void>;

struct Vec {
    int type = -1;
    bool scalar = false;   // literal broadcast
    double f = 0.0;
    long long i = 0;       // INT64 / INT32 / STRING code / BOOLEAN (0|1)
    Buf data;              // column values, or bitmap words for BOOLEAN
    Buf valid;             // known-bitmap, null = all valid
    std::shared_ptr<DictData> dict;
    bool is_str_lit = false;
    std::string lit;
    bool indexed = false;  // data = the BATCH column, to be read through the current domain's row ids (selection vector)
};

int kernel_type(int t) { return t == QE_STRING ? QE_INT32 : t; }

struct Exec {
    qe_ctx *ctx;
    hipStream_t s;
    int64_t n = 0;               // rows of the current domain
    std::vector<Vec> base;       // the batch's columns (full domain)
    std::vector<Vec> env;        // columns of the current domain; data == null: not gathered for it yet
    Buf ids;                     // u32 batch row ids of the current domain's rows (null: the domain is the whole batch)
    // batch columns whose ONLY remaining use is as a direct operand of an arithmetic node of the projections: the node reads
    // them through the row ids (a selection vector) instead of a gathered copy that is written once and read once
    std::vector<char> through_ids;
    int ieee;

    // column j in the current domain: gathered from the batch when a node first needs it here
    const Vec &column(int j) {
        const Vec &b = base[(size_t)j];
        if (!ids) return b;          // whole batch: the column itself (never cached: narrowing would re-gather it for nothing)
        Vec &v = env[(size_t)j];
        if (v.data) return v;
        v.type = b.type;
        v.dict = b.dict;
        if (b.type == QE_BOOLEAN) {
            v.data = alloc_words();
            launch_gather_bits_rows(s, (const uint64_t *)b.data.get(), (const uint32_t *)ids.get(), n, (uint64_t *)v.data.get());
        } else {
            v.data = alloc_col(b.type);
            pn::GatherArgs ga{};
            ga.idx = (const uint32_t *)ids.get();
            ga.m = n;
            ga.src[0] = b.data.get();
            ga.dst[0] = v.data.get();
            ga.width[0] = (int)type_width(b.type);
            ga.ncols = 1;
            pn::gather_multi(s, ga);
        }
        if (b.valid) {
            v.valid = alloc_words();
            launch_gather_bits_rows(s, (const uint64_t *)b.valid.get(), (const uint32_t *)ids.get(), n, (uint64_t *)v.valid.get());
        }
        return v;
    }

    // the value columns in `cols` that the current (narrowed) domain has not gathered yet: ONE launch, the ids are read once
    void prefetch(const std::vector<char> &cols) {
        if (!ids || n <= 0) return;
        pn::GatherArgs ga{};
        ga.idx = (const uint32_t *)ids.get();
        ga.m = n;
        auto flush = [&]() {
            if (ga.ncols > 0) pn::gather_multi(s, ga);
            ga.ncols = 0;
        };
        for (size_t j = 0; j < env.size(); j++) {
            if (!cols[j] || env[j].data || base[j].type == QE_BOOLEAN) continue;
            if (j < through_ids.size() && through_ids[j]) continue;
            Vec &v = env[j];
            v.type = base[j].type;
            v.dict = base[j].dict;
            v.data = alloc_col(base[j].type);
            ga.src[ga.ncols] = base[j].data.get();
            ga.dst[ga.ncols] = v.data.get();
            ga.width[ga.ncols] = (int)type_width(base[j].type);
            if (++ga.ncols == 8) flush();
            if (base[j].valid) {
                v.valid = alloc_words();
                launch_gather_bits_rows(s, (const uint64_t *)base[j].valid.get(), (const uint32_t *)ids.get(), n, (uint64_t *)v.valid.get());
            }
        }
        flush();
    }

    // narrow the domain to its rows rel[0..m) (ascending positions inside the current domain)
    void narrow(const Buf &rel, int64_t m) {
        const uint32_t *r = (const uint32_t *)rel.get();
        const int64_t old_n = n;
        (void)old_n;
        n = m;
        // the row ids and every value column the old domain had gathered move to the new one in ONE launch (the positions
        // `rel` are read once)
        pn::GatherArgs ga{};
        ga.idx = r;
        ga.m = m;
        std::vector<Buf> keep_alive;
        auto flush = [&]() {
            if (ga.ncols > 0) pn::gather_multi(s, ga);
            ga.ncols = 0;
        };
        if (ids) {
            Buf nids = alloc((size_t)std::max<int64_t>(m, 1) * 4);
            ga.src[ga.ncols] = ids.get();
            ga.dst[ga.ncols] = nids.get();
            ga.width[ga.ncols] = 4;
            ga.ncols++;
            keep_alive.push_back(ids);   // the old ids stay allocated until the gather has been launched
            ids = nids;
        } else {
            ids = rel;
        }
        for (size_t j = 0; j < env.size(); j++) {
            Vec &v = env[j];
            if (!v.data) continue;           // never needed so far: gathered from the batch if a later node asks for it
            Vec c;
            c.type = v.type;
            c.dict = v.dict;
            if (v.type == QE_BOOLEAN) {
                c.data = alloc_words();
                launch_gather_bits_rows(s, (const uint64_t *)v.data.get(), r, m, (uint64_t *)c.data.get());
            } else {
                c.data = alloc_col(v.type);
                ga.src[ga.ncols] = v.data.get();
                ga.dst[ga.ncols] = c.data.get();
                ga.width[ga.ncols] = (int)type_width(v.type);
                keep_alive.push_back(v.data);   // the source stays allocated until its gather has been launched
                if (++ga.ncols == 8) flush();
            }
            if (v.valid) {
                c.valid = alloc_words();
                launch_gather_bits_rows(s, (const uint64_t *)v.valid.get(), r, m, (uint64_t *)c.valid.get());
            }
            v = c;
        }
        flush();
    }

    Buf alloc(size_t bytes) {
        void *p = ctx->pool.alloc(bytes);
        qe_ctx *c = ctx;
        return Buf(p, [c](void *q) { c->pool.release(q); });
    }
    Buf alloc_col(int type) { return alloc(type_width(type) * (size_t)n); }   // value columns only: a BOOLEAN is alloc_words()
    Buf alloc_words() { return alloc(bitmap_bytes(n)); }

    pn::Opnd opnd(const Vec &v) {
        pn::Opnd o;
        o.ptr = v.scalar ? nullptr : v.data.get();
        o.f = v.f;
        o.i = v.i;
        o.idx = v.indexed ? (const uint32_t *)ids.get() : nullptr;
        return o;
    }

    // literal -> column / bitmap
    Vec materialize(const Vec &v) {
        if (!v.scalar) return v;
        Vec r = v;
        r.scalar = false;
        if (v.type == QE_BOOLEAN) {
            r.data = alloc_words();
            pn::word_fill(s, v.i ? ~0ull : 0ull, (uint64_t *)r.data.get(), bitmap_words(n));
        } else {
            r.data = alloc_col(v.type);
            pn::fill(s, kernel_type(v.type), opnd(v), r.data.get(), n);
        }
        return r;
    }

    Buf and_valid(const Buf &a, const Buf &b) {
        if (!a) return b;
        if (!b) return a;
        Buf r = alloc_words();
        pn::word_op(s, pn::W_AND, (const uint64_t *)a.get(), (const uint64_t *)b.get(), (uint64_t *)r.get(), bitmap_words(n));
        return r;
    }

    // map a STRING code column through a host table (string ranks, code remaps) -> INT32 column
    std::vector<std::shared_ptr<std::vector<int32_t>>> keep_tables;   // host staging must outlive the async copies
    Buf lookup(const std::vector<int32_t> &table, const Vec &codes) {
        auto host = std::make_shared<std::vector<int32_t>>(table);
        keep_tables.push_back(host);
        Buf dev = alloc(host->size() * 4);
        if (!host->empty()) QE_HIP(hipMemcpyAsync(dev.get(), host->data(), host->size() * 4, hipMemcpyHostToDevice, s));
        Buf out = alloc_col(QE_INT32);
        pn::lookup_codes(s, (const int32_t *)dev.get(), (int32_t)host->size(), (const int32_t *)codes.data.get(), (int32_t *)out.get(), n);
        keep_dev.push_back(dev);
        return out;
    }
    std::vector<Buf> keep_dev;

    // a plan constant table (membership bits / hash set) on the device
    Buf upload(const std::vector<int32_t> &table) {
        auto host = std::make_shared<std::vector<int32_t>>(table);
        keep_tables.push_back(host);
        Buf dev = alloc(std::max<size_t>(host->size() * 4, 16));
        if (!host->empty()) QE_HIP(hipMemcpyAsync(dev.get(), host->data(), host->size() * 4, hipMemcpyHostToDevice, s));
        keep_dev.push_back(dev);
        return dev;
    }

    // IN / LIKE: carries plan_member out.  Every route that is no constant goes through a table (a compare chain is an economy of
    // the fused kernel's text only): pn::member_bits or pn::member_hash.  The result shares the value's validity words.
    Vec member(const Expr &e, int id) {
        const Node &nd = e.nodes[id];
        const Node &vn = e.nodes[nd.ops[0]];
        Vec r;
        r.type = QE_BOOLEAN;
        int int_node = -1;
        if (vn.kind == N_CAST && vn.type == QE_DOUBLE) {
            const Node &c = e.nodes[vn.ops[0]];
            if ((c.type == QE_INT64 || c.type == QE_INT32) && c.kind != N_NUM) int_node = vn.ops[0];
        }
        MemberPlan mp;
        Vec a;
        if (vn.type == QE_STRING && vn.kind == N_COLUMN) {   // a folded test asks the column for its validity only
            mp = plan_member(e, id, StrSide{base[(size_t)vn.col].dict.get(), nullptr}, -1);
            if (mp.kind == MemberPlan::Constant) {
                r.scalar = true;
                r.i = mp.value ? 1 : 0;
                r.valid = validity(e, nd.ops[0]);
                return r;
            }
            a = eval(e, nd.ops[0]);
        } else if (vn.type == QE_STRING) {
            a = eval(e, nd.ops[0]);
            mp = plan_member(e, id, side(a), -1);
        } else {
            mp = plan_member(e, id, StrSide{nullptr, nullptr}, int_node >= 0 ? e.nodes[int_node].type : -1);
            a = eval(e, mp.on_int ? int_node : nd.ops[0]);
        }
        r.valid = a.valid;
        switch (mp.kind) {
        case MemberPlan::Constant:
            r.scalar = true;
            r.i = mp.value ? 1 : 0;
            return r;
        case MemberPlan::Copy: a.valid = r.valid; return a;
        case MemberPlan::Negate:
            a = materialize(a);
            r.data = alloc_words();
            pn::word_not(s, (const uint64_t *)a.data.get(), (uint64_t *)r.data.get(), bitmap_words(n));
            return r;
        default: break;
        }
        a = materialize(a);
        const int kt = kernel_type(a.type);
        r.data = alloc_words();
        if (mp.kind == MemberPlan::Bits) {
            pn::member_bits(s, kt, a.data.get(), mp.base, mp.nbits, (const uint32_t *)upload(mp.table).get(), (uint64_t *)r.data.get(), n);
            return r;
        }
        if (mp.kind == MemberPlan::Chain) {   // the same members as a hash set
            const MemberHashSet hs = build_member_hash(std::vector<uint64_t>(mp.chain.begin(), mp.chain.end()));
            mp.table.clear();
            for (uint64_t w : hs.words) {
                mp.table.push_back((int32_t)(uint32_t)w);
                mp.table.push_back((int32_t)(uint32_t)(w >> 32));
            }
        }
        pn::member_hash(s, kt, a.data.get(), (const uint64_t *)upload(mp.table).get(), (uint64_t *)r.data.get(), n);
        return r;
    }

    Buf ones() {
        Buf r = alloc_words();
        pn::word_fill(s, ~0ull, (uint64_t *)r.get(), bitmap_words(n));
        return r;
    }

    // operand `oid` of an arithmetic / comparison node: a batch column marked in `through_ids` is handed over as the column
    // itself plus the domain's row ids (a selection vector) when the domain is narrowed and holds no copy of it
    Vec operand(const Expr &e, int oid) {
        const Node &on = e.nodes[oid];
        if (on.kind == N_COLUMN && ids && through_ids[(size_t)on.col] && !env[(size_t)on.col].data) {
            Vec v = base[(size_t)on.col];   // non-owning: read as column[ids[j]]
            v.indexed = true;
            return v;
        }
        return eval(e, oid);
    }

    static StrSide side(const Vec &x) { return x.is_str_lit ? StrSide{nullptr, &x.lit} : StrSide{x.dict.get(), nullptr}; }

    // carries unify_dictionaries out: literals become their codes, the second side's codes are remapped (lookup_codes) where it says so
    std::shared_ptr<DictData> unify(Vec &t, Vec &f) {
        const DictUnion u = unify_dictionaries(side(t), side(f));
        if (u.remap_second) f.data = lookup(u.remap, f);
        if (t.is_str_lit) { t.i = u.lit[0]; t.is_str_lit = false; }
        if (f.is_str_lit) { f.i = u.lit[1]; f.is_str_lit = false; }
        return u.dict;
    }

    // validity words of node `oid` in the current domain (null: it cannot be NULL) WITHOUT its values: a batch column in a
    // narrowed domain has only its bitmap gathered
    Buf validity(const Expr &e, int oid) {
        const Node &on = e.nodes[oid];
        if (on.kind == N_COLUMN) {
            const Vec &b = base[(size_t)on.col];
            if (!ids || !b.valid) return b.valid;
            if (env[(size_t)on.col].data) return env[(size_t)on.col].valid;
            Buf k = alloc_words();
            launch_gather_bits_rows(s, (const uint64_t *)b.valid.get(), (const uint32_t *)ids.get(), n, (uint64_t *)k.get());
            return k;
        }
        return eval(e, oid).valid;
    }

    Vec eval(const Expr &e, int id) {
        const Node &nd = e.nodes[id];
        Vec r;
        r.type = nd.type;
        switch (nd.kind) {
        case N_COLUMN: return column(nd.col);   // (index and type: checked by column_uses before the first launch)
        case N_NUM: r.scalar = true; r.f = nd.num; return r;
        case N_BOOL: r.scalar = true; r.i = nd.bval ? 1 : 0; return r;
        case N_STR: r.is_str_lit = true; r.lit = nd.str; r.scalar = true; return r;
        case N_CAST: {
            Vec a = eval(e, nd.ops[0]);
            r.valid = a.valid;
            if (a.scalar) {   // literals are DOUBLE already; kept for completeness
                r.scalar = true;
                r.f = a.type == QE_DOUBLE ? a.f : (double)a.i;
                r.i = a.i;
                return r;
            }
            r.data = alloc_col(nd.type);
            pn::cast(s, a.type, nd.type, a.data.get(), r.data.get(), n);
            return r;
        }
        case N_FN: break;
        default: fail(QE_ERR_INTERNAL, "bad node kind");
        }

        switch (nd.fn) {
        case QE_FN_UNARY_PLUS: return eval(e, nd.ops[0]);
        case QE_FN_UNARY_MINUS: {
            Vec a = materialize(eval(e, nd.ops[0]));
            r.valid = a.valid;
            r.data = alloc_col(nd.type);
            pn::negate(s, nd.type, a.data.get(), r.data.get(), n);
            return r;
        }
        case QE_FN_ADD: case QE_FN_SUB: case QE_FN_MUL: case QE_FN_DIV: case QE_FN_MOD: {
            Vec a = operand(e, nd.ops[0]), b = operand(e, nd.ops[1]);
            if (a.scalar && b.scalar) a = materialize(a);
            r.valid = and_valid(a.valid, b.valid);
            const int op = nd.fn == QE_FN_ADD ? pn::A_ADD : nd.fn == QE_FN_SUB ? pn::A_SUB : nd.fn == QE_FN_MUL ? pn::A_MUL
                         : nd.fn == QE_FN_DIV ? pn::A_DIV : pn::A_MOD;
            if (nd.type != QE_DOUBLE && (op == pn::A_DIV || op == pn::A_MOD)) {
                Buf nz = alloc_words();   // integer division by zero => NULL
                pn::nonzero(s, nd.type, opnd(b), (uint64_t *)nz.get(), n);
                r.valid = and_valid(r.valid, nz);
            }
            r.data = alloc_col(nd.type);
            pn::arith(s, nd.type, op, opnd(a), opnd(b), r.data.get(), n);
            return r;
        }
        case QE_FN_CMP_LT: case QE_FN_CMP_LE: case QE_FN_CMP_GE: case QE_FN_CMP_GT: case QE_FN_CMP_EQ: case QE_FN_CMP_NE: {
            const int cmp = nd.fn == QE_FN_CMP_LT ? pn::C_LT : nd.fn == QE_FN_CMP_LE ? pn::C_LE : nd.fn == QE_FN_CMP_GE ? pn::C_GE
                          : nd.fn == QE_FN_CMP_GT ? pn::C_GT : nd.fn == QE_FN_CMP_EQ ? pn::C_EQ : pn::C_NE;
            const int ot = e.nodes[nd.ops[0]].type;
            if (ot == QE_DOUBLE) {
                // (double)int_column OP integral literal that exact_integer_literal accepts: compared on the integers -- no cast
                // kernel, no 8-byte temporary.  The compare kernel runs at the column's width: the literal must fit an INT32 column.
                auto int_child = [&](int id) {
                    const Node &x = e.nodes[id];
                    if (x.kind != N_CAST || x.type != QE_DOUBLE) return -1;
                    const Node &c = e.nodes[x.ops[0]];
                    return ((c.type == QE_INT64 || c.type == QE_INT32) && c.kind != N_NUM) ? x.ops[0] : -1;
                };
                auto int_lit = [&](int id, int ctype, long long &v) {
                    const Node &x = e.nodes[id];
                    return x.kind == N_NUM && exact_integer_literal(x.num, v) && (ctype == QE_INT64 || (v >= -2147483648ll && v <= 2147483647ll));
                };
                const int ia = int_child(nd.ops[0]), ib = int_child(nd.ops[1]);
                long long lit = 0;
                const bool left = ia >= 0 && int_lit(nd.ops[1], e.nodes[ia].type, lit);
                const bool right = !left && ib >= 0 && int_lit(nd.ops[0], e.nodes[ib].type, lit);
                if (left || right) {
                    Vec col = eval(e, left ? ia : ib), k;
                    if (!col.scalar) {
                        k.type = col.type;
                        k.scalar = true;
                        k.i = lit;
                        r.valid = col.valid;
                        r.data = alloc_words();
                        pn::compare(s, col.type, cmp, 0, left ? opnd(col) : opnd(k), left ? opnd(k) : opnd(col), (uint64_t *)r.data.get(), n);
                        return r;
                    }
                }
            }
            const bool numeric = ot == QE_DOUBLE || ot == QE_INT64 || ot == QE_INT32;
            Vec a = numeric ? operand(e, nd.ops[0]) : eval(e, nd.ops[0]), b = numeric ? operand(e, nd.ops[1]) : eval(e, nd.ops[1]);
            r.valid = and_valid(a.valid, b.valid);
            if (ot == QE_STRING) {
                const StringCompare sc = plan_string_compare(nd.fn, side(a), side(b));
                if (sc.kind == StringCompare::Constant) {
                    r.scalar = true;
                    r.i = sc.value ? 1 : 0;
                    return r;
                }
                Vec *x[2] = {&a, &b};
                for (int i = 0; i < 2; i++) {   // a literal side: its code / rank; a dictionary side: its codes, or their ranks as an INT32 column
                    if (x[i]->is_str_lit) { x[i]->i = sc.lit[i]; x[i]->is_str_lit = false; }
                    else if (sc.kind == StringCompare::Ranks) x[i]->data = lookup(sc.table[i], *x[i]);
                }
                r.data = alloc_words();
                pn::compare(s, QE_INT32, cmp, 0, opnd(a), opnd(b), (uint64_t *)r.data.get(), n);
                return r;
            }
            if (ot == QE_BOOLEAN) {   // Boolean.compare on bitmaps: false < true
                Vec x = materialize(a), y = materialize(b);
                const int w = cmp == pn::C_EQ ? pn::W_XNOR : cmp == pn::C_NE ? pn::W_XOR : cmp == pn::C_LT ? pn::W_NOTAND
                            : cmp == pn::C_LE ? pn::W_NOTOR : cmp == pn::C_GT ? pn::W_ANDNOT : pn::W_ORNOT;
                r.data = alloc_words();
                pn::word_op(s, w, (const uint64_t *)x.data.get(), (const uint64_t *)y.data.get(), (uint64_t *)r.data.get(), bitmap_words(n));
                return r;
            }
            if (a.scalar && b.scalar) a = materialize(a);
            r.data = alloc_words();
            pn::compare(s, ot, cmp, ieee, opnd(a), opnd(b), (uint64_t *)r.data.get(), n);
            return r;
        }
        case QE_FN_NOT: {   // ClosureCompiler.kt:115: null -> null
            Vec a = materialize(eval(e, nd.ops[0]));
            r.valid = a.valid;
            r.data = alloc_words();
            pn::word_not(s, (const uint64_t *)a.data.get(), (uint64_t *)r.data.get(), bitmap_words(n));
            return r;
        }
        case QE_FN_AND: case QE_FN_OR: {
            Vec a = materialize(eval(e, nd.ops[0])), b = materialize(eval(e, nd.ops[1]));
            r.data = alloc_words();
            if (a.valid || b.valid) r.valid = alloc_words();
            pn::kleene(s, nd.fn == QE_FN_AND, (const uint64_t *)a.data.get(), (const uint64_t *)a.valid.get(),
                       (const uint64_t *)b.data.get(), (const uint64_t *)b.valid.get(), (uint64_t *)r.data.get(),
                       (uint64_t *)r.valid.get(), bitmap_words(n));
            return r;
        }
        case QE_FN_IF: {   // Interpreter.kt:46-53: null condition -> null; both branches evaluated, then selected
            Vec c = materialize(eval(e, nd.ops[0])), t = eval(e, nd.ops[1]), f = eval(e, nd.ops[2]);
            Buf cond = c.data;
            if (c.valid) cond = and_valid(c.data, c.valid);   // c = vc & kc
            if (nd.type == QE_STRING) r.dict = unify(t, f);
            if (nd.type == QE_BOOLEAN) {
                Vec tt = materialize(t), ff = materialize(f);
                r.data = alloc_words();
                pn::select_words(s, (const uint64_t *)cond.get(), (const uint64_t *)tt.data.get(), (const uint64_t *)ff.data.get(),
                                 (uint64_t *)r.data.get(), bitmap_words(n));
            } else {
                r.data = alloc_col(nd.type);
                pn::select(s, kernel_type(nd.type), (const uint64_t *)cond.get(), opnd(t), opnd(f), r.data.get(), n);
            }
            if (t.valid || f.valid) {
                Buf kt = t.valid ? t.valid : ones(), kf = f.valid ? f.valid : ones();
                Buf sel = alloc_words();
                pn::select_words(s, (const uint64_t *)cond.get(), (const uint64_t *)kt.get(), (const uint64_t *)kf.get(),
                                 (uint64_t *)sel.get(), bitmap_words(n));
                r.valid = and_valid(c.valid, sel);
            } else {
                r.valid = c.valid;
            }
            return r;
        }
        case QE_FN_IS_NULL: case QE_FN_IS_NOT_NULL: {   // word operations on the operand's validity; its data is never read
            const Buf k = validity(e, nd.ops[0]);
            const bool is_null = nd.fn == QE_FN_IS_NULL;
            r.data = alloc_words();
            if (!k) pn::word_fill(s, is_null ? 0ull : ~0ull, (uint64_t *)r.data.get(), bitmap_words(n));
            else if (is_null) pn::word_not(s, (const uint64_t *)k.get(), (uint64_t *)r.data.get(), bitmap_words(n));
            else if (n > 0) QE_HIP(hipMemcpyAsync(r.data.get(), k.get(), bitmap_bytes(n), hipMemcpyDeviceToDevice, s));
            return r;
        }
        case QE_FN_COALESCE: {   // select on the first operand's validity words; NULL iff both operands are
            Vec a = eval(e, nd.ops[0]), b = eval(e, nd.ops[1]);
            if (!a.valid) return a;   // never NULL: the node is its first operand
            if (nd.type == QE_STRING) r.dict = unify(a, b);
            if (nd.type == QE_BOOLEAN) {
                Vec bb = materialize(b);
                r.data = alloc_words();
                pn::select_words(s, (const uint64_t *)a.valid.get(), (const uint64_t *)a.data.get(), (const uint64_t *)bb.data.get(),
                                 (uint64_t *)r.data.get(), bitmap_words(n));
            } else {
                r.data = alloc_col(nd.type);
                pn::select(s, kernel_type(nd.type), (const uint64_t *)a.valid.get(), opnd(a), opnd(b), r.data.get(), n);
            }
            if (b.valid) {
                r.valid = alloc_words();
                pn::word_op(s, pn::W_OR, (const uint64_t *)a.valid.get(), (const uint64_t *)b.valid.get(), (uint64_t *)r.valid.get(), bitmap_words(n));
            }
            return r;
        }
        case QE_FN_ABS: case QE_FN_FLOOR: case QE_FN_CEIL: {
            Vec a = eval(e, nd.ops[0]);
            if (nd.fn != QE_FN_ABS && nd.type != QE_DOUBLE) return a;   // an integer is its own floor and ceiling
            a = materialize(a);
            r.valid = a.valid;
            r.data = alloc_col(nd.type);
            pn::unary(s, nd.type, nd.fn == QE_FN_ABS ? pn::U_ABS : nd.fn == QE_FN_FLOOR ? pn::U_FLOOR : pn::U_CEIL, a.data.get(), r.data.get(), n);
            return r;
        }
        case QE_FN_IN: case QE_FN_LIKE: return member(e, id);
        default: fail(QE_ERR_INTERNAL, "bad function");
        }
    }
};

}  // namespace

qe_result *run_per_node(qe_ctx *ctx, const qe_batch *batch, const qe_expr *filter, const qe_expr *const *projs,
                        int32_t nproj) {
    if (nproj < 0 || (nproj > 0 && !projs)) fail(QE_ERR_INVALID_ARG, "bad projection list");
    if (batch->nrows >= (1ll << 31)) fail(QE_ERR_UNSUPPORTED, "QE_EXEC_PER_NODE uses 32-bit row ids: batch too large");
    Exec x;
    x.ctx = ctx;
    x.s = ctx->stream;
    x.n = batch->nrows;
    x.ieee = ctx->opts.cmp_semantics == QE_CMP_IEEE;
    for (const Column &c : batch->cols) {
        Vec v;
        v.type = c.type;
        v.data = Buf(c.data, [](void *) {});
        if (c.validity) v.valid = Buf(c.validity, [](void *) {});
        v.dict = c.dict;
        x.base.push_back(v);
        Vec e;
        e.type = c.type;
        e.dict = c.dict;
        x.env.push_back(e);          // not gathered yet
    }
    ResultPtr res = new_result(ctx, 0);   // (its columns share their buffers with the executor's temporaries: hold_data / hold_valid)
    int64_t m = batch->nrows;
    // A value column that the whole plan uses exactly once, as a direct operand of an arithmetic or comparison node, is never
    // gathered into a narrowed domain: the node reads it through the row ids (cfg 2: `a + b` after the filter -- 0.8 GB less
    // written and 0.8 GB less read per 1 B rows; cfg 3: `l_quantity < 24`, `l_extendedprice * ..`).
    std::vector<char> proj_values(x.env.size(), 0);   // columns whose VALUES the projections read (a null test asks for the validity only)
    {
        std::vector<int> col_types, refs(x.env.size(), 0), direct(x.env.size(), 0);
        for (const Column &c : batch->cols) col_types.push_back(c.type);
        auto scan = [&](const Expr &pe, bool projection) {
            std::vector<std::shared_ptr<DictData>> dicts;
            for (const Column &c : batch->cols) dicts.push_back(c.dict);
            const std::vector<char> folded = constant_column_members(pe, dicts);   // an IN / LIKE folded to a constant reads the validity only
            for (const ColumnUse &u : column_uses(pe, pe.root, col_types, &folded)) {   // (raises the plan's column errors before the first launch)
                refs[(size_t)u.col]++;
                if (projection && u.value) proj_values[(size_t)u.col] = 1;
            }
            for (const Node &nd : pe.nodes)
                if (nd.kind == N_FN && (is_arithmetic_fn(nd.fn) || is_comparison_fn(nd.fn)))
                    for (int op : nd.ops)
                        if (pe.nodes[(size_t)op].kind == N_COLUMN) direct[(size_t)pe.nodes[(size_t)op].col]++;
        };
        if (filter) scan(filter->e, false);
        for (int32_t i = 0; i < nproj; i++) {
            if (!projs[i]) fail(QE_ERR_INVALID_ARG, "null projection");
            scan(projs[i]->e, true);
        }
        x.through_ids.assign(x.env.size(), 0);
        for (size_t j = 0; j < x.env.size(); j++)
            x.through_ids[j] = refs[j] == 1 && direct[j] == 1 && !x.base[j].valid &&
                               (x.base[j].type == QE_DOUBLE || x.base[j].type == QE_INT64 || x.base[j].type == QE_INT32);
    }
    if (ctx->opts.profile) QE_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    if (filter && batch->nrows > 0) {
        const Expr &fe = filter->e;
        if (fe.nodes[fe.root].type != QE_BOOLEAN) fail(QE_ERR_PROGRAM, "filter expression must be BOOLEAN");
        const std::vector<int> conj = split_conjuncts(fe, fe.root);   // 1. the top-level AND chain, left to right
        unsigned long long *d_total = (unsigned long long *)(ctx->d_ctrl + 2);
        Buf acc;   // keep mask accumulated over the conjuncts evaluated in the current domain since it was last narrowed
        for (size_t ci = 0; ci < conj.size() && x.n > 0; ci++) {
            const bool last = ci + 1 == conj.size();
            Vec k = x.materialize(x.eval(fe, conj[ci]));
            Buf keep = x.and_valid(k.data, k.valid);              // value & known (FilterOperator.kt:20)
            acc = x.and_valid(acc, keep);
            // 2. kept rows of the current domain
            const int64_t nw = bitmap_words(x.n);
            Buf offsets = x.alloc((size_t)(nw + 1) * 4), sums = x.alloc((size_t)scan_blocks(nw + 1) * 4);
            bitmap_ranks(x.s, (const uint64_t *)acc.get(), nullptr, x.n, (uint32_t *)offsets.get(), (uint32_t *)sums.get(), d_total);
            QE_HIP(hipMemcpyAsync(ctx->h_ctrl, ctx->d_ctrl, 16, hipMemcpyDeviceToHost, x.s));
            QE_HIP(hipGetLastError());
            QE_HIP(hipStreamSynchronize(x.s));
            const int64_t kept = (int64_t)ctx->h_ctrl[1];
            if (last && ctx->opts.result_capacity_rows > 0 && kept > ctx->opts.result_capacity_rows)   // same contract as the fused path
                fail(QE_ERR_INVALID_ARG, "result has " + std::to_string(kept) + " rows but result_capacity_rows is " +
                                             std::to_string(ctx->opts.result_capacity_rows));
            if (kept == x.n) { acc.reset(); continue; }           // everything survived: the domain stays as it is
            if (!last && kept * 2 > x.n) continue;                // not selective enough to pay for a compaction yet: keep the mask
            Buf rel = x.alloc((size_t)std::max<int64_t>(kept, 1) * 4);
            bitmap_positions(x.s, (const uint64_t *)acc.get(), nullptr, x.n, (const uint32_t *)offsets.get(), (uint32_t *)rel.get(), kept, false);
            x.narrow(rel, kept);
            acc.reset();
        }
        m = x.n;
        // 3. the projections' columns that the final domain has not seen yet: one gather launch
        x.prefetch(proj_values);
    }
    // 4. projections over the (compacted) domain
    res->count = m;
    res->capacity = m;
    for (int32_t i = 0; i < nproj; i++) {
        const Expr &pe = projs[i]->e;
        Vec v = x.eval(pe, pe.root);
        if (v.is_str_lit) {   // SELECT 'lit'
            v.dict = literal_dictionary(v.lit);
            v.i = 0;
            v.is_str_lit = false;
        }
        if (m > 0) v = x.materialize(v);
        OutColumn oc;
        oc.type = v.type;
        oc.dict = v.dict;
        oc.dict_handle.d = v.dict;
        oc.nullable = (bool)v.valid;
        if (m > 0) {
            // a bare column of an unfiltered batch aliases the caller's input: the result must own its data
            auto owned = [&](const Buf &b, size_t bytes) -> Buf {
                if (!b) return b;
                for (const Column &c : batch->cols)
                    if (b.get() == c.data || b.get() == (void *)c.validity) {
                        Buf copy = x.alloc(bytes);
                        QE_HIP(hipMemcpyAsync(copy.get(), b.get(), bytes, hipMemcpyDeviceToDevice, x.s));
                        return copy;
                    }
                return b;
            };
            const size_t dbytes = column_bytes(v.type, m);
            oc.hold_data = owned(v.data, dbytes);
            oc.hold_valid = owned(v.valid, bitmap_bytes(m));
            oc.data = oc.hold_data.get();
            oc.validity = (uint64_t *)oc.hold_valid.get();
        }
        res->cols.push_back(oc);
    }
    if (ctx->opts.profile) QE_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    QE_HIP(hipGetLastError());
    QE_HIP(hipStreamSynchronize(x.s));
    if (ctx->opts.profile) {
        float ms = 0.f;
        QE_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        ctx->last_ms = ms;
        ctx->total_ms += ms;
        ctx->launches++;
    }
    return res.release();
}

}  // namespace qe
