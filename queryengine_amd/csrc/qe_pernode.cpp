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
#include <cstring>
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

// what a buffer holds, as the launchers take it
uint64_t *words(const Buf &b) { return (uint64_t *)b.get(); }   // bitmap words: BOOLEAN values, validity; hash-set words
uint32_t *u32(const Buf &b) { return (uint32_t *)b.get(); }     // row ids, scan offsets, 32-bit table words
int32_t *codes(const Buf &b) { return (int32_t *)b.get(); }     // dictionary codes, INT32 tables

// Value columns to be gathered at the same row ids idx[0..m): one pn::gather_multi per `per_launch` (at most 8) of them, which
// reads the ids once.  A source stays allocated until the batch is gone, that is until its gather has been launched.
struct Gather {
    hipStream_t s;
    int per_launch;
    pn::GatherArgs ga{};
    std::vector<Buf> held;
    Gather(hipStream_t s, const uint32_t *idx, int64_t m, int per_launch = 8) : s(s), per_launch(per_launch) {
        ga.idx = idx;
        ga.m = m;
    }
    void add(const Buf &src, const Buf &dst, int width) {
        ga.src[ga.ncols] = src.get();
        ga.dst[ga.ncols] = dst.get();
        ga.width[ga.ncols] = width;
        held.push_back(src);
        if (++ga.ncols == per_launch) flush();
    }
    void flush() {
        if (ga.ncols > 0) pn::gather_multi(s, ga);
        ga.ncols = 0;
    }
};

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

    // `src` (a column of the batch, or of the domain being left) at the row ids of the batch `g`: a value column joins g's next
    // launch; a BOOLEAN column and the validity words are bitmap gathers of their own.  n is the row count of the NEW domain.
    Vec gathered(const Vec &src, Gather &g) {
        Vec c;
        c.type = src.type;
        c.dict = src.dict;
        if (src.type == QE_BOOLEAN) {
            c.data = alloc_words();
            launch_gather_bits_rows(s, words(src.data), g.ga.idx, n, words(c.data));
        } else {
            c.data = alloc_col(src.type);
            g.add(src.data, c.data, (int)type_width(src.type));
        }
        if (src.valid) {
            c.valid = alloc_words();
            launch_gather_bits_rows(s, words(src.valid), g.ga.idx, n, words(c.valid));
        }
        return c;
    }

    // column j in the current domain: gathered from the batch when a node first needs it here
    const Vec &column(int j) {
        const Vec &b = base[(size_t)j];
        if (!ids) return b;          // whole batch: the column itself (never cached: narrowing would re-gather it for nothing)
        Vec &v = env[(size_t)j];
        if (!v.data) {
            Gather g(s, u32(ids), n, 1);
            v = gathered(b, g);
        }
        return v;
    }

    // the value columns in `cols` that the current (narrowed) domain has not gathered yet: ONE launch, the ids are read once
    void prefetch(const std::vector<char> &cols) {
        if (!ids || n <= 0) return;
        Gather g(s, u32(ids), n);
        for (size_t j = 0; j < env.size(); j++) {
            if (!cols[j] || env[j].data || base[j].type == QE_BOOLEAN) continue;
            if (j < through_ids.size() && through_ids[j]) continue;
            env[j] = gathered(base[j], g);
        }
        g.flush();
    }

    // narrow the domain to its rows rel[0..m) (ascending positions inside the current domain)
    void narrow(const Buf &rel, int64_t m) {
        n = m;
        // the row ids and every value column the old domain had gathered move to the new one in ONE launch (the positions
        // `rel` are read once)
        Gather g(s, u32(rel), m);
        if (ids) {
            Buf nids = alloc((size_t)std::max<int64_t>(m, 1) * 4);
            g.add(ids, nids, 4);
            ids = nids;
        } else {
            ids = rel;
        }
        for (Vec &v : env)
            if (v.data) v = gathered(v, g);   // (never needed so far: gathered from the batch if a later node asks for it)
        g.flush();
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
        o.idx = v.indexed ? u32(ids) : nullptr;
        return o;
    }

    // literal -> column / bitmap
    Vec materialize(const Vec &v) {
        if (!v.scalar) return v;
        Vec r = v;
        r.scalar = false;
        if (v.type == QE_BOOLEAN) {
            r.data = alloc_words();
            pn::word_fill(s, v.i ? ~0ull : 0ull, words(r.data), bitmap_words(n));
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
        pn::word_op(s, pn::W_AND, words(a), words(b), words(r), bitmap_words(n));
        return r;
    }

    // A host table on the device: string ranks and code remaps, membership bits and hash-set words.  The host copy must outlive
    // the async copy and the device buffer the kernels that read it: both are held until the executor is gone.  The host copy
    // lies in the context's pinned pool, not in malloc's memory: with a 1 MiB hash set there, an execution took 19 ms where
    // malloc mapped the block afresh and 36 - 48 ms where it grew the heap for it and trimmed the heap again afterwards, and
    // which of the two a process did followed from its earlier allocations (profiles/pernode_evaluator_refactor_summary.txt).
    struct Staged { Buf host, dev; };
    std::vector<Staged> staged;
    Buf upload(const std::vector<int32_t> &table) {
        const size_t bytes = table.size() * 4;
        qe_ctx *c = ctx;
        Staged t{Buf(ctx->pinned.alloc(bytes), [c](void *q) { c->pinned.release(q); }), alloc(std::max<size_t>(bytes, 16))};
        if (bytes > 0) {
            std::memcpy(t.host.get(), table.data(), bytes);
            QE_HIP(hipMemcpyAsync(t.dev.get(), t.host.get(), bytes, hipMemcpyHostToDevice, s));
        }
        staged.push_back(t);
        return t.dev;
    }
    // a STRING code column mapped through such a table -> INT32 column
    Buf lookup(const std::vector<int32_t> &table, const Vec &v) {
        Buf dev = upload(table), out = alloc_col(QE_INT32);
        pn::lookup_codes(s, codes(dev), (int32_t)table.size(), codes(v.data), codes(out), n);
        return out;
    }

    // IN / LIKE: carries plan_member out.  Every route that is no constant goes through a table (a compare chain is an economy of
    // the fused kernel's text only): pn::member_bits or pn::member_hash.  The result shares the value's validity words.
    Vec member(const Expr &e, int id) {
        const Node &nd = e.nodes[id];
        const Node &vn = e.nodes[nd.ops[0]];
        Vec r;
        r.type = QE_BOOLEAN;
        const int int_node = integer_cast_operand(e, nd.ops[0]);
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
            pn::word_not(s, words(a.data), words(r.data), bitmap_words(n));
            return r;
        default: break;
        }
        a = materialize(a);
        const int kt = kernel_type(a.type);
        r.data = alloc_words();
        if (mp.kind == MemberPlan::Bits) {
            pn::member_bits(s, kt, a.data.get(), mp.base, mp.nbits, u32(upload(mp.table)), words(r.data), n);
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
        pn::member_hash(s, kt, a.data.get(), words(upload(mp.table)), words(r.data), n);
        return r;
    }

    Buf ones() {
        Buf r = alloc_words();
        pn::word_fill(s, ~0ull, words(r), bitmap_words(n));
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
            launch_gather_bits_rows(s, words(b.valid), u32(ids), n, words(k));
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
                pn::nonzero(s, nd.type, opnd(b), words(nz), n);
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
                // (double)int_column OP integral literal that exact_integer_literal accepts at the column's width: compared on
                // the integers -- no cast kernel, no 8-byte temporary
                auto int_lit = [&](int id, int ctype, long long &v) {
                    const Node &x = e.nodes[id];
                    return x.kind == N_NUM && exact_integer_literal(x.num, ctype, v);
                };
                const int ia = integer_cast_operand(e, nd.ops[0]), ib = integer_cast_operand(e, nd.ops[1]);
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
                        pn::compare(s, col.type, cmp, 0, left ? opnd(col) : opnd(k), left ? opnd(k) : opnd(col), words(r.data), n);
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
                pn::compare(s, QE_INT32, cmp, 0, opnd(a), opnd(b), words(r.data), n);
                return r;
            }
            if (ot == QE_BOOLEAN) {   // Boolean.compare on bitmaps: false < true
                Vec x = materialize(a), y = materialize(b);
                const int w = cmp == pn::C_EQ ? pn::W_XNOR : cmp == pn::C_NE ? pn::W_XOR : cmp == pn::C_LT ? pn::W_NOTAND
                            : cmp == pn::C_LE ? pn::W_NOTOR : cmp == pn::C_GT ? pn::W_ANDNOT : pn::W_ORNOT;
                r.data = alloc_words();
                pn::word_op(s, w, words(x.data), words(y.data), words(r.data), bitmap_words(n));
                return r;
            }
            if (a.scalar && b.scalar) a = materialize(a);
            r.data = alloc_words();
            pn::compare(s, ot, cmp, ieee, opnd(a), opnd(b), words(r.data), n);
            return r;
        }
        case QE_FN_NOT: {   // ClosureCompiler.kt:115: null -> null
            Vec a = materialize(eval(e, nd.ops[0]));
            r.valid = a.valid;
            r.data = alloc_words();
            pn::word_not(s, words(a.data), words(r.data), bitmap_words(n));
            return r;
        }
        case QE_FN_AND: case QE_FN_OR: {
            Vec a = materialize(eval(e, nd.ops[0])), b = materialize(eval(e, nd.ops[1]));
            r.data = alloc_words();
            if (a.valid || b.valid) r.valid = alloc_words();
            pn::kleene(s, nd.fn == QE_FN_AND, words(a.data), words(a.valid),
                       words(b.data), words(b.valid), words(r.data),
                       words(r.valid), bitmap_words(n));
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
                pn::select_words(s, words(cond), words(tt.data), words(ff.data),
                                 words(r.data), bitmap_words(n));
            } else {
                r.data = alloc_col(nd.type);
                pn::select(s, kernel_type(nd.type), words(cond), opnd(t), opnd(f), r.data.get(), n);
            }
            if (t.valid || f.valid) {
                Buf kt = t.valid ? t.valid : ones(), kf = f.valid ? f.valid : ones();
                Buf sel = alloc_words();
                pn::select_words(s, words(cond), words(kt), words(kf),
                                 words(sel), bitmap_words(n));
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
            if (!k) pn::word_fill(s, is_null ? 0ull : ~0ull, words(r.data), bitmap_words(n));
            else if (is_null) pn::word_not(s, words(k), words(r.data), bitmap_words(n));
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
                pn::select_words(s, words(a.valid), words(a.data), words(bb.data),
                                 words(r.data), bitmap_words(n));
            } else {
                r.data = alloc_col(nd.type);
                pn::select(s, kernel_type(nd.type), words(a.valid), opnd(a), opnd(b), r.data.get(), n);
            }
            if (b.valid) {
                r.valid = alloc_words();
                pn::word_op(s, pn::W_OR, words(a.valid), words(b.valid), words(r.valid), bitmap_words(n));
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

    // ---- the plan, piece by piece (run_per_node) ---------------------------------------------------------------------------
    // Before the first launch: the plan's column errors, and which columns are read through the row ids.  A value column that
    // the whole plan uses exactly once, as a direct operand of an arithmetic or comparison node, is never gathered into a
    // narrowed domain: the node reads it through the row ids (cfg 2: `a + b` after the filter -- 0.8 GB less written and
    // 0.8 GB less read per 1 B rows; cfg 3: `l_quantity < 24`, `l_extendedprice * ..`).
    // Returns the columns whose VALUES the projections read (a null test asks for the validity only).
    std::vector<char> analyse(const qe_batch *batch, const qe_expr *filter, const qe_expr *const *projs, int32_t nproj) {
        std::vector<char> proj_values(env.size(), 0);
        std::vector<int> col_types, refs(env.size(), 0), direct(env.size(), 0);
        std::vector<std::shared_ptr<DictData>> dicts;
        for (const Column &c : batch->cols) {
            col_types.push_back(c.type);
            dicts.push_back(c.dict);
        }
        auto scan = [&](const Expr &pe, bool projection) {
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
        through_ids.assign(env.size(), 0);
        for (size_t j = 0; j < env.size(); j++)
            through_ids[j] = refs[j] == 1 && direct[j] == 1 && !base[j].valid &&
                             (base[j].type == QE_DOUBLE || base[j].type == QE_INT64 || base[j].type == QE_INT32);
        return proj_values;
    }

    // Steps 1 - 3 of the file comment: the filter, conjunct by conjunct, leaves the domain at the kept rows
    void filter_domain(const Expr &fe, const std::vector<char> &proj_values) {
        if (fe.nodes[fe.root].type != QE_BOOLEAN) fail(QE_ERR_PROGRAM, "filter expression must be BOOLEAN");
        const std::vector<int> conj = split_conjuncts(fe, fe.root);   // 1. the top-level AND chain, left to right
        unsigned long long *d_total = (unsigned long long *)(ctx->d_ctrl + 2);
        Buf acc;   // keep mask accumulated over the conjuncts evaluated in the current domain since it was last narrowed
        for (size_t ci = 0; ci < conj.size() && n > 0; ci++) {
            const bool last = ci + 1 == conj.size();
            Vec k = materialize(eval(fe, conj[ci]));
            Buf keep = and_valid(k.data, k.valid);              // value & known (FilterOperator.kt:20)
            acc = and_valid(acc, keep);
            // 2. kept rows of the current domain
            const int64_t nw = bitmap_words(n);
            Buf offsets = alloc((size_t)(nw + 1) * 4), sums = alloc((size_t)scan_blocks(nw + 1) * 4);
            bitmap_ranks(s, words(acc), nullptr, n, u32(offsets), u32(sums), d_total);
            QE_HIP(hipMemcpyAsync(ctx->h_ctrl, ctx->d_ctrl, 16, hipMemcpyDeviceToHost, s));
            QE_HIP(hipGetLastError());
            QE_HIP(hipStreamSynchronize(s));
            const int64_t kept = (int64_t)ctx->h_ctrl[1];
            if (last && ctx->opts.result_capacity_rows > 0 && kept > ctx->opts.result_capacity_rows)   // same contract as the fused path
                fail(QE_ERR_INVALID_ARG, "result has " + std::to_string(kept) + " rows but result_capacity_rows is " +
                                             std::to_string(ctx->opts.result_capacity_rows));
            if (kept == n) { acc.reset(); continue; }           // everything survived: the domain stays as it is
            if (!last && kept * 2 > n) continue;                // not selective enough to pay for a compaction yet: keep the mask
            Buf rel = alloc((size_t)std::max<int64_t>(kept, 1) * 4);
            bitmap_positions(s, words(acc), nullptr, n, u32(offsets), u32(rel), kept, false);
            narrow(rel, kept);
            acc.reset();
        }
        // 3. the projections' columns that the final domain has not seen yet: one gather launch
        prefetch(proj_values);
    }

    // Step 4: one projection over the final domain, as a column of the result (which shares the buffer with the executor's
    // temporaries: hold_data / hold_valid)
    OutColumn project(const Expr &pe, const qe_batch *batch) {
        Vec v = eval(pe, pe.root);
        if (v.is_str_lit) {   // SELECT 'lit'
            v.dict = literal_dictionary(v.lit);
            v.i = 0;
            v.is_str_lit = false;
        }
        OutColumn oc;
        oc.type = v.type;
        oc.dict = v.dict;
        oc.dict_handle.d = v.dict;
        oc.nullable = (bool)v.valid;
        if (n <= 0) return oc;
        v = materialize(v);
        // a bare column of an unfiltered batch aliases the caller's input: the result must own its data
        auto owned = [&](const Buf &b, size_t bytes) -> Buf {
            if (!b) return b;
            for (const Column &c : batch->cols)
                if (b.get() == c.data || b.get() == (void *)c.validity) {
                    Buf copy = alloc(bytes);
                    QE_HIP(hipMemcpyAsync(copy.get(), b.get(), bytes, hipMemcpyDeviceToDevice, s));
                    return copy;
                }
            return b;
        };
        oc.hold_data = owned(v.data, column_bytes(v.type, n));
        oc.hold_valid = owned(v.valid, bitmap_bytes(n));
        oc.data = oc.hold_data.get();
        oc.validity = words(oc.hold_valid);
        return oc;
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
    ResultPtr res = new_result(ctx, 0);
    const std::vector<char> proj_values = x.analyse(batch, filter, projs, nproj);
    if (ctx->opts.profile) QE_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    if (filter && batch->nrows > 0) x.filter_domain(filter->e, proj_values);
    res->count = x.n;
    res->capacity = x.n;
    for (int32_t i = 0; i < nproj; i++) res->cols.push_back(x.project(projs[i]->e, batch));
    if (ctx->opts.profile) QE_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    QE_HIP(hipGetLastError());
    QE_HIP(hipStreamSynchronize(x.s));
    collect_time(ctx);   // (the bracket ev0 .. ev1, when profiling)
    return res.release();
}

}  // namespace qe
