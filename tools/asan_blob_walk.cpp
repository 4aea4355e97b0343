/* Development tool: the blob entries of the C ABI (gpu_batch.hip, "bulk pack / unpack") walked by a plain program, so that the
 * host code of that section runs under AddressSanitizer without Python in the process.  Linked with the kernel sources under the
 * host-simulation shim (tests/hostsim): the "device" arrays are heap blocks, an element outside its array is reported with its line.
 *     cd tests/hostsim && mkdir -p ../../tools/ab && g++ -O1 -g -fsanitize=address -fno-omit-frame-pointer -std=c++17 -x c++ -Wno-unknown-pragmas -Iinclude \
 *         -I../../include -I../../acados_amd/csrc ../../tools/asan_blob_walk.cpp ../../acados_amd/csrc/gpu_batch.hip \
 *         ../../acados_amd/csrc/gpu_shapes_large.hip ../../acados_amd/csrc/ocp_qp_host.cpp ../../acados_amd/csrc/ocp_qp_xcond.cpp \
 *         -o ../../tools/ab/asan_blob_walk && ../../tools/ab/asan_blob_walk
 * 70 instances (one full tile and a ragged one) of a small structure with an equality-flagged x0, box bounds and soft state bounds;
 * the cases of tests/test_blob_layout.py: (a) _set_bulk_vec leaves the matrices, (b) _set_bulk_out / _get_bulk, (c) bulk seeds against
 * the per-field seeds; besides them the chunk protocol and the data gradient (grad_build reads the host tables of the output map).
 * Exit code 0 and "asan_blob_walk: ok" when every comparison held. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "acados_amd/ocp_qp_gpu_batch.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "asan_blob_walk: FAILED at line %d: %s\n", __LINE__, #x); exit(1); } } while (0)

static const int N = 3, NX = 2, NU = 1, B = 70;
static unsigned long long rng_state = 88172645463325252ull;
static double rnd() /* xorshift, uniform in (-1, 1) */
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (double) (rng_state >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}

static void set_all(ocp_qp_gpu_batch *b, const char *f, int k, const std::vector<double> &one, double jitter = 0.0)
{
    std::vector<double> v((size_t) B * one.size());
    for (int i = 0; i < B; i++) for (size_t e = 0; e < one.size(); e++) v[i * one.size() + e] = one[e] + jitter * rnd();
    CHECK(ocp_qp_gpu_batch_set(b, f, k, v.data(), 0) == 0);
}

struct Seg { std::string f; int k, off, len; };

static std::vector<Seg> segments(ocp_qp_gpu_batch *b, int sens, int output, const std::vector<std::string> &fields)
{
    std::vector<Seg> s;
    for (int k = 0; k <= N; k++)
        for (const std::string &f : fields)
        {
            int len = 0;
            const int off = sens ? ocp_qp_gpu_batch_sens_bulk_offset(b, output, f.c_str(), k, &len) : ocp_qp_gpu_batch_bulk_offset(b, output, f.c_str(), k, &len);
            if (off >= 0 && len > 0) s.push_back(Seg{f, k, off, len});
        }
    return s;
}

int main()
{
    /* stage 0: x0 fixed (equality-flagged bounds on both states), u boxed; stages 1 .. N: soft bounds on both states; u boxed below N */
    const int nx[N + 1] = {NX, NX, NX, NX}, nu[N + 1] = {NU, NU, NU, 0}, nbx[N + 1] = {NX, NX, NX, NX}, nbu[N + 1] = {NU, NU, NU, 0};
    const int ng[N + 1] = {0, 0, 0, 0}, ns[N + 1] = {0, NX, NX, NX};
    ocp_qp_gpu_batch *b = ocp_qp_gpu_batch_create(N, nx, nu, nbx, nbu, ng, ns, B, -1);
    CHECK(b);
    for (int k = 0; k <= N; k++)
    {
        std::vector<int> idxb, rev;
        for (int j = 0; j < nu[k] + NX; j++) idxb.push_back(j);
        for (int j = 0; j < nbu[k]; j++) rev.push_back(-1);
        for (int j = 0; j < NX; j++) rev.push_back(k ? j : -1);
        CHECK(ocp_qp_gpu_batch_set_int(b, "idxb", k, idxb.data(), (int) idxb.size()) == 0);
        if (k) CHECK(ocp_qp_gpu_batch_set_int(b, "idxs_rev", k, rev.data(), (int) rev.size()) == 0);
    }
    const int idxe[2] = {NU, NU + 1};
    CHECK(ocp_qp_gpu_batch_set_int(b, "idxe", 0, idxe, 2) == 0);
    for (int k = 0; k <= N; k++)
    {
        if (k < N)
        {
            set_all(b, "A", k, {1.0, 0.0, 0.1, 1.0}, 0.01);
            set_all(b, "B", k, {0.005, 0.1}, 0.01);
            set_all(b, "b", k, {0.0, 0.0}, 0.01);
            set_all(b, "R", k, {0.5});
            set_all(b, "S", k, {0.0, 0.0});
            set_all(b, "r", k, {0.0}, 0.1);
            set_all(b, "lbu", k, {-0.5});
            set_all(b, "ubu", k, {0.5});
        }
        set_all(b, "Q", k, {1.0, 0.0, 0.0, 1.0});
        set_all(b, "q", k, {0.0, 0.0}, 0.1);
        if (k == 0) { set_all(b, "lbx", k, {1.0, 0.5}, 0.2); }
        else
        {
            set_all(b, "lbx", k, {-0.6, -0.6});
            set_all(b, "ubx", k, {0.6, 0.6});
            set_all(b, "Zl", k, {10.0, 10.0}); set_all(b, "Zu", k, {10.0, 10.0});
            set_all(b, "zl", k, {1.0, 1.0}); set_all(b, "zu", k, {1.0, 1.0});
            set_all(b, "lls", k, {0.0, 0.0}); set_all(b, "lus", k, {0.0, 0.0});
        }
    }
    {   /* ubx of the fixed x0 = its lbx */
        std::vector<double> x0((size_t) B * NX);
        CHECK(ocp_qp_gpu_batch_get(b, "lbx", 0, x0.data(), 0) == 0);
        CHECK(ocp_qp_gpu_batch_set(b, "ubx", 0, x0.data(), 0) == 0);
    }
    const std::vector<std::string> in_f = {"A", "B", "b", "Q", "S", "R", "q", "r", "lbu", "ubu", "lbx", "lbx#value", "ubx", "lg", "ug", "C", "D", "Zl", "Zu", "zl", "zu",
                                           "lls", "lus", "lbu_mask", "ubu_mask", "lbx_mask", "ubx_mask", "lg_mask", "ug_mask", "lls_mask", "lus_mask"};
    const std::vector<std::string> out_f = {"u", "x", "sl", "su", "pi", "lam", "t"};
    const int n_in = ocp_qp_gpu_batch_bulk_len(b, 0), n_out = ocp_qp_gpu_batch_bulk_len(b, 1), n_vec = ocp_qp_gpu_batch_bulk_len(b, 2);
    CHECK(n_in > 0 && n_out > 0 && n_vec > 0 && n_vec < n_in && ocp_qp_gpu_batch_bulk_len(b, 3) == n_out);
    std::vector<double> ref((size_t) B * n_in), back((size_t) B * n_in);
    CHECK(ocp_qp_gpu_batch_get_bulk_in(b, ref.data(), 0) == 0);

    /* whole, and in chunks: the same data back */
    CHECK(ocp_qp_gpu_batch_set_bulk(b, ref.data(), 0) == 0);
    CHECK(ocp_qp_gpu_batch_get_bulk_in(b, back.data(), 0) == 0 && back == ref);
    CHECK(ocp_qp_gpu_batch_set_bulk_staged(b) == -1);
    CHECK(ocp_qp_gpu_batch_set_bulk_chunk(b, ref.data(), 0, 33) == 0);
    CHECK(ocp_qp_gpu_batch_set_bulk_chunk(b, ref.data() + (size_t) 33 * n_in, 33, B - 33) == 0);
    CHECK(ocp_qp_gpu_batch_set_bulk_staged(b) == 0);
    CHECK(ocp_qp_gpu_batch_get_bulk_in(b, back.data(), 0) == 0 && back == ref);

    /* (a) new vectors and masks: the matrices stay, the vectors are what was sent */
    {
        std::vector<double> vec((size_t) B * n_vec, 0.0);
        const std::vector<Seg> vs = segments(b, 0, 2, in_f), is = segments(b, 0, 0, in_f);
        for (const Seg &s : vs)
            for (int i = 0; i < B; i++)
                for (int e = 0; e < s.len; e++)
                {
                    double &v = vec[(size_t) i * n_vec + s.off + e];
                    if (s.f.size() > 5 && s.f.compare(s.f.size() - 5, 5, "_mask") == 0) v = (s.k == 0 && s.f[2] == 'x') || rnd() < 0.6 ? 1.0 : 0.0;
                    else if (s.f == "lbx#value") v = vec[(size_t) i * n_vec + s.off - s.len + e];
                    else v = rnd();
                }
        CHECK(ocp_qp_gpu_batch_set_bulk_vec(b, vec.data(), 0) == 0);
        CHECK(ocp_qp_gpu_batch_get_bulk_in(b, back.data(), 0) == 0);
        for (const Seg &s : is)
        {
            const Seg *v = nullptr;
            for (const Seg &q : vs) if (q.f == s.f && q.k == s.k) v = &q;
            if (s.f == "lbx#value" && s.k != 0) continue; /* no equality-flagged row: the entries refer to nothing */
            for (int i = 0; i < B; i++)
                for (int e = 0; e < s.len; e++)
                {
                    const double got = back[(size_t) i * n_in + s.off + e];
                    if (v) CHECK(v->len == s.len && got == vec[(size_t) i * n_vec + v->off + e]);
                    else CHECK(got == ref[(size_t) i * n_in + s.off + e]);
                }
        }
        CHECK(ocp_qp_gpu_batch_set_bulk(b, ref.data(), 0) == 0);
    }

    /* (b) an iterate in, the same iterate out */
    {
        std::vector<double> it((size_t) B * n_out), got((size_t) B * n_out);
        for (double &v : it) v = rnd();
        CHECK(ocp_qp_gpu_batch_set_bulk_out(b, it.data(), 0) == 0);
        CHECK(ocp_qp_gpu_batch_get_bulk(b, got.data(), 0) == 0 && got == it);
        CHECK(ocp_qp_gpu_batch_get_bulk(b, got.data(), 1) == 0 && got == it); /* (host simulation: any pointer is a device pointer) */
    }

    /* (c) bulk seeds against the per-field seeds, at the solution */
    CHECK(ocp_qp_gpu_batch_solve(b) == 0);
    {
        std::vector<std::string> seed_f, sens_f;
        for (const char *f : {"r", "q", "zl", "zu", "b", "lbu", "lbx", "lg", "ubu", "ubx", "ug", "lls", "lus"}) seed_f.push_back(std::string("seed_") + f);
        for (const std::string &f : out_f) sens_f.push_back("sens_" + f);
        const int n_seed = ocp_qp_gpu_batch_sens_bulk_len(b, 0);
        CHECK(n_seed > 0 && ocp_qp_gpu_batch_sens_bulk_len(b, 1) == n_out);
        std::vector<double> seeds((size_t) B * n_seed), single((size_t) B * n_out, 0.0), bulk((size_t) B * n_out, 0.0);
        for (double &v : seeds) v = rnd();
        for (const Seg &s : segments(b, 1, 0, seed_f))
        {
            std::vector<double> part((size_t) B * s.len);
            for (int i = 0; i < B; i++) memcpy(&part[(size_t) i * s.len], &seeds[(size_t) i * n_seed + s.off], sizeof(double) * s.len);
            CHECK(ocp_qp_gpu_batch_sens_set(b, s.f.c_str(), s.k, part.data()) == 0);
        }
        CHECK(ocp_qp_gpu_batch_sens_solve(b) == 0);
        for (const Seg &s : segments(b, 1, 1, sens_f))
        {
            std::vector<double> part((size_t) B * s.len);
            CHECK(ocp_qp_gpu_batch_get(b, s.f.c_str(), s.k, part.data(), 0) == 0);
            for (int i = 0; i < B; i++) memcpy(&single[(size_t) i * n_out + s.off], &part[(size_t) i * s.len], sizeof(double) * s.len);
        }
        CHECK(ocp_qp_gpu_batch_sens_set_bulk(b, seeds.data(), 0) == 0);
        CHECK(ocp_qp_gpu_batch_sens_solve(b) == 0);
        CHECK(ocp_qp_gpu_batch_sens_get_bulk(b, bulk.data(), 0) == 0);
        CHECK(memcmp(bulk.data(), single.data(), sizeof(double) * bulk.size()) == 0);
        double mx = 0.0;
        for (double v : bulk) mx = v > mx ? v : (-v > mx ? -v : mx);
        CHECK(mx > 0.0);
    }

    /* the data gradient: grad_build renumbers the output map from its host tables */
    {
        std::vector<double> cot((size_t) B * n_out, 0.0), grad((size_t) B * n_in, 0.0);
        for (const Seg &s : segments(b, 0, 1, {"u", "x", "sl", "su"}))
            for (int i = 0; i < B; i++) for (int e = 0; e < s.len; e++) cot[(size_t) i * n_out + s.off + e] = rnd();
        CHECK(ocp_qp_gpu_batch_adj_seed_bulk(b, cot.data(), 0) == 0);
        CHECK(ocp_qp_gpu_batch_data_grad_bulk(b, grad.data(), 0) == 0);
        double mx = 0.0;
        for (double v : grad) { CHECK(v == v); mx = v > mx ? v : (-v > mx ? -v : mx); }
        CHECK(mx > 0.0);
        /* ... and with a cotangent on every entry of the output blob: seed_all_build walks the seed map and the output map */
        std::vector<double> all((size_t) B * n_out), grad_all((size_t) B * n_in, 0.0);
        for (double &v : all) v = rnd();
        CHECK(ocp_qp_gpu_batch_adj_seed_all_bulk(b, all.data(), 0) == 0);
        CHECK(ocp_qp_gpu_batch_data_grad_bulk(b, grad_all.data(), 0) == 0);
        for (double v : grad_all) CHECK(v == v);
        CHECK(memcmp(grad_all.data(), grad.data(), sizeof(double) * grad.size()) != 0);
        CHECK(ocp_qp_gpu_batch_adj_seed_all_bulk(b, cot.data(), 0) == 0);
        CHECK(ocp_qp_gpu_batch_data_grad_bulk(b, grad_all.data(), 0) == 0);
        CHECK(memcmp(grad_all.data(), grad.data(), sizeof(double) * grad.size()) == 0); /* zero on pi lam t: the bits of _adj_seed_bulk */
    }
    CHECK(ocp_qp_gpu_batch_get_scalar(b, "time_pack") >= 0.0);
    ocp_qp_gpu_batch_destroy(b);
    printf("asan_blob_walk: ok\n");
    return 0;
}
