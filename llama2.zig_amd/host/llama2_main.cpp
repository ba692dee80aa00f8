// llama2_main.cpp -- the reference's command line (src/main.zig:800-1051) over the
// MI355X forward pass.  Same flags, defaults, clamping, output and tokens/s rule;
// transformer() runs on the GPU through include/llama2_hip.h.
//
//   llama2 <checkpoint> [-t temp] [-p top_p] [-n steps] [-i prompt] [-s seed] [-v] [-z tokenizer]
//          [-g n_gpus]   (extension: rows / heads sharded over n GPUs, one process per GPU)
//          [-b n]        (extension: n independent samples of the prompt, stepped together: run_batch)
//          [--score]     (extension: no generation -- the log-prob of every prompt token and the perplexity: run_score)
//          [--spec K]    (extension, -t 0 only: speculative greedy decoding -- up to K tokens guessed by prompt lookup are
//                         verified per sweep of the weights by l2z_verify; the text does not depend on K: run_spec)
//          [--spec-sample K]  (extension: the same under the run's -t / -p / -s by l2z_verify_sample: a guess is accepted
//                         when it is the token the sampler draws with that position's own random number: run_spec)
//
// At -t 0 the whole generation loop runs on the device (l2z_greedy_run) and the host
// only prints; otherwise one l2z_transformer + l2z_logits_read per position feeds the
// reference's host-side samplers.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/llama2_hip.h"
#include "llama2_host.hpp"

using namespace l2zhost;

// main.zig:800-813
static const char *usage_text =
    "Usage:   llama2 <checkpoint> [options]\n"
    "Example: llama2 checkpoint.bin -n 256 -i \"Once upon a time\"\n"
    "Options:\n"
    " -h, --help                print this help message\n"
    " -t, --temperature <float> temperature, default 1.0 (0.0, 1]\n"
    " -p, --top-p <float>       p value in top-p (nucleus) sampling. default 0.9, 0 || 1 = off\n"
    " -n, --seq-len <int>       number of steps to run for, default 256. 0 = max_seq_len\n"
    " -i, --input <string>      input text for the prompt, default \"\"\n"
    " -s, --seed <int>          random seed, default to time\n"
    " -v, --verbose             print model info and tokens/s\n"
    " -z, --tokenizer <path>    path to the tokenizer to use, default to \"tokenizer.bin\"\n"
    " --tokens                  (extension) also print the token ids to stderr, one line\n"
    " -g, --gpus <int>          (extension) shard weight rows / heads over this many GPUs, default 1\n"
    " -b, --batch <int>         (extension) generate this many independent samples of the prompt together, 1-16,\n"
    "                           default 1; sample i draws from seed + i\n"
    " --score                   (extension) generate nothing: print pos, token id, piece, log-prob and top-1 id of every\n"
    "                           token of the prompt (-i), then tokens, nll/token and perplexity; not with -g or -b\n"
    " --spec <int>              (extension) speculative greedy decoding, needs -t 0: guess up to this many tokens (0-15) by\n"
    "                           looking the last tokens up in the text so far, verify them in one pass; the text is the same\n"
    "                           for every value.  A pass of one token costs ~1.25x a plain -t 0 step, so it pays on text that\n"
    "                           repeats its context; not with -b, -g or --score\n"
    " --spec-sample <int>       (extension) speculative decoding under the sampler (-t, -p, -s as given): guess up to this\n"
    "                           many tokens (0-15) as --spec does; a guess is accepted when it is the token the sampler\n"
    "                           draws with that position's own random number, so the text is the same for every value and\n"
    "                           its law is the plain sampler's.  At -t 0 it is --spec; not with --spec, -b, -g or --score\n";

static bool verbose = false;
#define LOGV(...)                                 \
    do {                                          \
        if (verbose) fprintf(stderr, __VA_ARGS__); \
    } while (0)

static int die(const char *what)
{
    fprintf(stderr, "error: %s: %s\n", what, l2z_last_error());
    return 1;
}

// ---- -g N: one process per GPU.  The parent is rank 0 and forks ranks 1..N-1 BEFORE
// anything touches the GPU; every rank maps the checkpoint itself and uploads only its own rows
// (l2z_weights_init with a comm), the ranks exchange the 64-byte IPC handles of their landing
// arenas through files in a private temporary directory, and then all of them run the very same
// generation loop -- same tokens in, bit-identical logits out, so they stay in step
// without talking to each other; only rank 0 prints.
static int g_rank = 0, g_world = 1;

// A rank that cannot take part (comm_init / p2p_export failed on its GPU) leaves an error marker so that
// the others stop waiting at once instead of polling for its handle for a minute.
static void mark_failed(const std::string &dir)
{
    if (dir.empty()) return;
    FILE *f = fopen((dir + "/e" + std::to_string(g_rank)).c_str(), "wb");
    if (f) fclose(f);
}

static bool any_rank_failed(const std::string &dir, const std::vector<pid_t> &kids)
{
    for (int r = 0; r < g_world; r++)
        if (access((dir + "/e" + std::to_string(r)).c_str(), F_OK) == 0) return true;
    for (pid_t k : kids) {  // rank 0 only: a child that has already gone will never write its handle
        siginfo_t si;
        si.si_pid = 0;
        if (waitid(P_PID, (id_t)k, &si, WEXITED | WNOHANG | WNOWAIT) == 0 && si.si_pid == k) return true;
    }
    return false;
}

static bool exchange_handles(const std::string &dir, const std::vector<pid_t> &kids, const void *mine,
                             std::vector<char> *all)
{
    const std::string tmp = dir + "/h" + std::to_string(g_rank) + ".tmp", fin = dir + "/h" + std::to_string(g_rank);
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f) return false;
    const bool wrote = fwrite(mine, 1, L2Z_COMM_IPC_BYTES, f) == L2Z_COMM_IPC_BYTES;
    if (fclose(f) != 0 || !wrote) return false;
    if (rename(tmp.c_str(), fin.c_str()) != 0) return false;
    all->resize((size_t)g_world * L2Z_COMM_IPC_BYTES);
    for (int r = 0; r < g_world; r++) {
        const std::string p = dir + "/h" + std::to_string(r);
        FILE *g = nullptr;
        for (int tries = 0; tries < 6000 && !(g = fopen(p.c_str(), "rb")); tries++) {
            if ((tries % 10) == 9 && any_rank_failed(dir, kids)) return false;
            usleep(10000);
        }
        if (!g) return false;
        const size_t n = fread(all->data() + (size_t)r * L2Z_COMM_IPC_BYTES, 1, L2Z_COMM_IPC_BYTES, g);
        fclose(g);
        if (n != L2Z_COMM_IPC_BYTES) return false;
    }
    return true;
}

// -b N, N >= 2: N independent samples of the prompt.  The prompt's positions run once, on s (one batched prefill where
// the sampled path of main() takes it, else stepped); l2z_runstate_fork copies them to N - 1 more runstates; then each
// position is one l2z_transformer_batch and one l2z_sample_batch over the samples still running.  A sample leaves at
// BOS (:1017) or at the -n limit.  Sample i draws its numbers from its own generator seeded seed + i, one per sampled
// token as :1009-1012 draw them, so sample 0 uses the stream of the run without -b.  The texts print when every sample
// has ended, each behind a line "--- sample i ---".
static int run_batch(int nb, const l2z_config &cfg, const l2z_weights *w, l2z_runstate *s, const Tokenizer &tok,
                     const std::vector<int32_t> &prompt, size_t seq_len, float temperature, float top_p, uint64_t seed,
                     bool dump_tokens)
{
    struct Sample {
        l2z_runstate *st = nullptr;
        Prng rng;
        std::string text;
        std::vector<int32_t> ids;
        size_t token = 1;  // last emitted (the input of the next position)
        bool alive = true;
    };
    std::vector<Sample> sm((size_t)nb);
    int rc = 0;
    sm[0].st = s;
    for (int i = 0; i < nb; i++) {
        sm[(size_t)i].rng.seed_with(seed + (uint64_t)i);
        if (i > 0 && rc == 0 && l2z_runstate_init(&cfg, nullptr, &sm[(size_t)i].st) != L2Z_OK) rc = die("RunState.init");
    }
    auto cleanup = [&](int r) {
        for (size_t i = 1; i < sm.size(); i++)
            if (sm[i].st) l2z_runstate_free(sm[i].st);
        return r;
    };
    if (rc) return cleanup(rc);
    // :1017-1034 for one sample: false when the sequence ended
    auto emit = [&](Sample &x, size_t next) -> bool {
        x.ids.push_back((int32_t)next);
        if (next == 1) return x.alive = false;
        std::string_view piece = tok.tokens[next];
        if (x.token == 1 && !piece.empty() && piece[0] == ' ') piece.remove_prefix(1);
        const int byte = is_raw_byte(piece);
        if (byte >= 0) x.text.push_back((char)byte);
        else x.text.append(piece.data(), piece.size());
        x.token = next;
        return true;
    };
    // the prompt positions (:999-1000): the same tokens in every sample
    const size_t n_prompt = std::min(prompt.size(), seq_len);
    for (Sample &x : sm)
        for (size_t p = 0; p < n_prompt && emit(x, (size_t)prompt[p]);) p++;
    size_t pos = n_prompt;
    if (sm[0].alive && pos < seq_len) {
        const char *pf_env = getenv("L2Z_PREFILL");
        std::vector<int32_t> in(n_prompt);
        for (size_t i = 0; i < n_prompt; i++) in[i] = i == 0 ? 1 : prompt[i - 1];
        size_t done = 0;
        if (n_prompt >= L2Z_PREFILL_MIN_PROMPT && !(pf_env && atoi(pf_env) == 0) &&
            l2z_prefill(in.data(), (int)n_prompt, 0, &cfg, s, w) == L2Z_OK)
            done = n_prompt;
        for (; done < n_prompt; done++)
            if (l2z_transformer(in[done], (int)done, &cfg, s, w) != L2Z_OK) return cleanup(die("transformer"));
        for (int i = 1; i < nb; i++)
            if (l2z_runstate_fork(sm[(size_t)i].st, s, (int)n_prompt) != L2Z_OK) return cleanup(die("runstate_fork"));
    }
    std::vector<l2z_runstate *> act_st;
    std::vector<int32_t> act_tok, act_pos, out;
    std::vector<float> temps, tops, coins;
    std::vector<size_t> act;
    size_t sampled = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (; pos < seq_len; pos++) {
        act.clear();
        for (size_t i = 0; i < sm.size(); i++)
            if (sm[i].alive) act.push_back(i);
        if (act.empty()) break;
        const size_t n = act.size();
        act_st.resize(n); act_tok.resize(n); act_pos.assign(n, (int32_t)pos); out.resize(n);
        temps.assign(n, temperature); tops.assign(n, top_p); coins.resize(n);
        for (size_t j = 0; j < n; j++) {
            Sample &x = sm[act[j]];
            act_st[j] = x.st;
            act_tok[j] = (int32_t)x.token;
            coins[j] = temperature == 0.0f ? 0.0f : x.rng.next_f32();  // :731 / :789, one number per sampled token
        }
        if (l2z_transformer_batch((int)n, act_tok.data(), act_pos.data(), &cfg, act_st.data(), w) != L2Z_OK)
            return cleanup(die("transformer_batch"));
        if (l2z_sample_batch((int)n, act_st.data(), temps.data(), tops.data(), coins.data(), out.data()) != L2Z_OK)
            return cleanup(die("sample_batch"));
        for (size_t j = 0; j < n; j++) emit(sm[act[j]], (size_t)out[j]);
        sampled += n;
    }
    for (size_t i = 0; i < sm.size(); i++) {
        printf("--- sample %zu ---\n", i);
        fwrite(sm[i].text.data(), 1, sm[i].text.size(), stdout);
        fputc('\n', stdout);
    }
    fflush(stdout);
    const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (sampled > 0) LOGV("\n%u tokens per second (%d samples together)\n", (unsigned)(el > 0.0 ? sampled / el : 0.0), nb);
    if (dump_tokens)
        for (size_t i = 0; i < sm.size(); i++) {
            fprintf(stderr, "tokens[%zu]:", i);
            for (int32_t t : sm[i].ids) fprintf(stderr, " %d", t);
            fprintf(stderr, "\n");
        }
    return cleanup(0);
}

// --score: the prompt as generation feeds it -- BOS, then its tokens (:999-1000) -- through one l2z_score call: position i
// reads token i of that sequence and is scored on prompt[i].  One line per position, then the totals (host double).  Where the
// library refuses the model's dims (L2Z_ERR_INVALID, as l2z_prefill does) the positions are stepped and the log-softmax is
// the host's; same output.
static int run_score(const l2z_config &cfg, const l2z_weights *w, l2z_runstate *s, const Tokenizer &tok,
                     const std::vector<int32_t> &prompt)
{
    const size_t n = prompt.size();
    if (n == 0) {
        fprintf(stderr, "error: --score needs a prompt (-i)\n");
        return 1;
    }
    if (n > (size_t)cfg.seq_len) {
        fprintf(stderr, "error: --score: the prompt has %zu tokens, the model's seq_len is %d\n", n, cfg.seq_len);
        return 1;
    }
    std::vector<int32_t> in(n), top1(n);
    std::vector<float> lp(n);
    for (size_t i = 0; i < n; i++) in[i] = i == 0 ? 1 : prompt[i - 1];
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = l2z_score(in.data(), (int)n, 0, prompt.data(), &cfg, s, w, lp.data(), top1.data());
    if (rc == L2Z_ERR_INVALID) {
        LOGV("score: %s -- stepping the positions\n", l2z_last_error());
        std::vector<float> z((size_t)cfg.vocab_size);
        for (size_t i = 0; i < n; i++) {
            if (l2z_transformer(in[i], (int)i, &cfg, s, w) != L2Z_OK) return die("transformer");
            if (l2z_logits_read(s, z.data()) != L2Z_OK) return die("logits_read");
            size_t best = 0;
            for (size_t v = 1; v < z.size(); v++)
                if (z[v] > z[best]) best = v;
            double sum = 0.0;
            for (float v : z) sum += std::exp((double)v - (double)z[best]);
            lp[i] = (float)((double)z[(size_t)prompt[i]] - ((double)z[best] + std::log(sum)));
            top1[i] = (int32_t)best;
        }
    } else if (rc != L2Z_OK) {
        return die("score");
    }
    const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    double total = 0.0;
    for (size_t i = 0; i < n; i++) {
        std::string piece = "\"";
        for (unsigned char ch : tok.tokens[(size_t)prompt[i]]) {
            char buf[8];
            if (ch == '"' || ch == '\\') { piece.push_back('\\'); piece.push_back((char)ch); }
            else if (ch < 0x20 || ch == 0x7f) { snprintf(buf, sizeof buf, "\\x%02x", ch); piece += buf; }
            else piece.push_back((char)ch);
        }
        piece.push_back('"');
        printf("%zu\t%d\t%s\t%.6f\t%d\n", i, prompt[i], piece.c_str(), (double)lp[i], top1[i]);
        total += (double)lp[i];
    }
    const double nll = -total / (double)n;
    printf("tokens: %zu\nnll/token: %.6f\nperplexity: %.6f\n", n, nll, std::exp(nll));
    fflush(stdout);
    LOGV("\n%u tokens per second (scored)\n", (unsigned)(el > 0.0 ? (double)n / el : 0.0));
    return 0;
}

// --spec K: the greedy loop of :995-1042 over l2z_verify.  The prompt (BOS, then its tokens) is one l2z_prefill, the first
// generated token l2z_argmax; then every call feeds the last token and up to K guesses (lookup_draft over everything emitted
// so far) and emits the 1 + accepted tokens it returns.  Steps without a guess, and K = 0, still go through l2z_verify with
// one row: the ids must not depend on the drafter, and l2z_transformer's bits differ from a verify row's at near-ties.
// --spec-sample K (draw != nullptr): the same loop over l2z_verify_sample with the run's temperature and top_p.  Generated
// token g is drawn with coin g of Prng(seed), whatever call draws it: the coins are taken from the generator lazily, in
// generation order, and KEPT -- a coin drawn for a row behind a rejected guess is the coin of that position in the next
// call.  The first generated token is l2z_sample_batch's draw from the prefill's logits with coin 0.  At -t 0 no coin is
// drawn and the calls are --spec's.
struct SpecDraw {
    float temperature, top_p;
    Prng *rng;
};
static int run_spec(int K, const l2z_config &cfg, const l2z_weights *w, l2z_runstate *s, const Tokenizer &tok,
                    const std::vector<int32_t> &prompt, size_t seq_len, bool dump_tokens, const SpecDraw *draw = nullptr)
{
    const bool sampled = draw != nullptr && draw->temperature != 0.0f;
    std::vector<float> coins;  // coins[g]: generated token g's
    size_t gen = 0;            // generated tokens so far
    auto coins_upto = [&](size_t n) {
        while (coins.size() < n) coins.push_back(draw->rng->next_f32());
    };
    std::vector<int32_t> hist{1}, produced;  // hist: the sequence as the model reads it (BOS first)
    size_t token = 1, pos = 0;
    bool timer_started = false;
    std::chrono::steady_clock::time_point t0;
    auto emit = [&](size_t next) -> bool {  // :1017-1041, as main()'s
        produced.push_back((int32_t)next);
        hist.push_back((int32_t)next);
        if (next == 1) return false;
        std::string_view piece = tok.tokens[next];
        if (token == 1 && !piece.empty() && piece[0] == ' ') piece.remove_prefix(1);
        const int byte = is_raw_byte(piece);
        token = next;
        if (byte >= 0) {
            fputc(byte, stdout);
            return true;
        }
        fwrite(piece.data(), 1, piece.size(), stdout);
        if (!timer_started) {
            fflush(stdout);
            timer_started = true;
            t0 = std::chrono::steady_clock::now();
        }
        return true;
    };
    bool alive = true;
    const size_t n_prompt = std::min(prompt.size(), seq_len);
    while (alive && pos < n_prompt) {  // :999-1000
        alive = emit((size_t)prompt[pos]);
        if (alive) pos++;
    }
    long calls = 0, offered = 0, accepted = 0, from_calls = 0;
    if (alive && pos < seq_len) {
        if (l2z_prefill(hist.data(), (int)hist.size(), 0, &cfg, s, w) != L2Z_OK) return die("prefill");
        int first = 0;
        if (sampled) {
            coins_upto(1);
            int32_t t = 0;
            if (l2z_sample_batch(1, &s, &draw->temperature, &draw->top_p, coins.data(), &t) != L2Z_OK) return die("sample_batch");
            first = t;
        } else if (l2z_argmax(s, &first) != L2Z_OK) {
            return die("argmax");
        }
        alive = emit((size_t)first);
        gen++;
        if (alive) pos++;
    }
    int32_t in[L2Z_BATCH_MAX], next[L2Z_BATCH_MAX];
    while (alive && pos < seq_len) {
        in[0] = (int32_t)token;
        const size_t room = seq_len - pos - 1;  // positions after this one that may still emit
        const int k = (int)std::min<size_t>((size_t)K, room);
        const int nd = (int)lookup_draft(hist.data(), hist.size(), 3, k, in + 1);
        int a = 0;
        if (draw != nullptr) {
            if (sampled) coins_upto(gen + 1 + (size_t)nd);
            if (l2z_verify_sample(in, 1 + nd, (int)pos, draw->temperature, draw->top_p, sampled ? coins.data() + gen : nullptr,
                                  &cfg, s, w, next, &a) != L2Z_OK)
                return die("verify_sample");
        } else if (l2z_verify(in, 1 + nd, (int)pos, &cfg, s, w, next, &a) != L2Z_OK) {
            return die("verify");
        }
        calls++; offered += nd; accepted += a;
        for (int i = 0; i <= a && alive && pos < seq_len; i++) {
            alive = emit((size_t)next[i]);
            from_calls++;
            gen++;
            if (alive) pos++;
        }
    }
    fflush(stdout);
    if (timer_started) {
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        LOGV("\n\n%u tokens per second\n", (unsigned)(pos >= 1 && el > 0.0 ? (double)(pos - 1) / el : 0.0));
    }
    LOGV("%s: %ld verify calls, %.2f tokens per call, %ld guesses offered, %ld accepted\n",
         draw != nullptr ? "spec-sample" : "spec", calls, calls ? (double)from_calls / (double)calls : 0.0, offered, accepted);
    if (dump_tokens) {
        fprintf(stderr, "tokens:");
        for (int32_t t : produced) fprintf(stderr, " %d", t);
        fprintf(stderr, "\n");
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) {  // :833-836
        fputs(usage_text, stdout);
        return 0;
    }
    const char *bin_path = nullptr;
    const char *input = nullptr;
    float temperature = 1.0f, top_p = 0.9f;  // :840-841
    size_t seq_len = 0;
    std::string tokenizer_path = "tokenizer.bin";
    bool dump_tokens = false, score = false;
    int n_gpus = 1, n_batch = 1, spec = -1, spec_sample = -1;
    uint64_t seed = (uint64_t)std::chrono::system_clock::now().time_since_epoch().count();
    Prng prng(seed);  // :844-845

    auto need = [&](int &i, const char *what) -> const char * {  // :863-867 etc.
        if (++i >= argc) {
            fprintf(stderr, "error: missing argument for %s\n", what);
            exit(1);
        }
        return argv[i];
    };
    for (int i = 1; i < argc; i++) {  // :848-934
        const std::string a = argv[i];
        if (a == "-h" || a == "--help") {
            fputs(usage_text, stdout);
            return 0;
        }
        if (a.empty() || a[0] != '-') {
            if (bin_path) {  // :856-858
                fprintf(stderr, "error: multiple checkpoint paths specified\n");
                return 1;
            }
            bin_path = argv[i];
        } else if (a == "-t" || a == "--temperature") {
            const char *v = need(i, "temperature");
            char *end = nullptr;
            temperature = strtof(v, &end);
            if (end == v || *end) {
                fprintf(stderr, "unable to parse --temperature argument '%s'\n", v);
                return 1;
            }  // not clamped, :874
        } else if (a == "-n" || a == "--seq-len") {
            const char *v = need(i, "seq-len");
            char *end = nullptr;
            const long long n = strtoll(v, &end, 10);
            if (end == v || *end || n < 0) {
                fprintf(stderr, "unable to parse --seq-len argument '%s'\n", v);
                return 1;
            }
            seq_len = (size_t)n;
        } else if (a == "-p" || a == "--top-p") {
            const char *v = need(i, "top-p");
            char *end = nullptr;
            top_p = strtof(v, &end);
            if (end == v || *end) {
                fprintf(stderr, "unable to parse --top-p argument '%s'\n", v);
                return 1;
            }
            top_p = top_p < 0.0f ? 0.0f : (top_p > 1.0f ? 1.0f : top_p);  // :899
        } else if (a == "-i" || a == "--input") {
            input = need(i, "input");
        } else if (a == "-z" || a == "--tokenizer") {
            tokenizer_path = need(i, "tokenizer");
        } else if (a == "-s" || a == "--seed") {
            const char *v = need(i, "seed");
            char *end = nullptr;
            const unsigned long long s = strtoull(v, &end, 10);
            if (end == v || *end) {
                fprintf(stderr, "unable to parse --seed argument '%s'\n", v);
                return 1;
            }
            seed = (uint64_t)s;
            prng.seed_with(seed);  // :926
        } else if (a == "-v" || a == "--verbose") {
            verbose = true;
        } else if (a == "--tokens") {
            dump_tokens = true;
        } else if (a == "--score") {
            score = true;
        } else if (a == "--spec") {
            const char *v = need(i, "spec");
            char *end = nullptr;
            const long k = strtol(v, &end, 10);
            if (end == v || *end || k < 0 || k > L2Z_BATCH_MAX - 1) {
                fprintf(stderr, "unable to use --spec argument '%s' (0 to %d)\n", v, L2Z_BATCH_MAX - 1);
                return 1;
            }
            spec = (int)k;
        } else if (a == "--spec-sample") {
            const char *v = need(i, "spec-sample");
            char *end = nullptr;
            const long k = strtol(v, &end, 10);
            if (end == v || *end || k < 0 || k > L2Z_BATCH_MAX - 1) {
                fprintf(stderr, "unable to use --spec-sample argument '%s' (0 to %d)\n", v, L2Z_BATCH_MAX - 1);
                return 1;
            }
            spec_sample = (int)k;
        } else if (a == "-g" || a == "--gpus") {
            n_gpus = atoi(need(i, "gpus"));
            if (n_gpus < 1 || n_gpus > 16) {
                fprintf(stderr, "unable to use --gpus argument '%s'\n", argv[i]);
                return 1;
            }
        } else if (a == "-b" || a == "--batch") {
            const char *v = need(i, "batch");
            char *end = nullptr;
            const long nb = strtol(v, &end, 10);
            if (end == v || *end || nb < 1 || nb > L2Z_BATCH_MAX) {
                fprintf(stderr, "unable to use --batch argument '%s' (1 to %d)\n", v, L2Z_BATCH_MAX);
                return 1;
            }
            n_batch = (int)nb;
        } else {  // :929-933
            fprintf(stderr, "error: unknown argument '%s'\n", argv[i]);
            fputs(usage_text, stdout);
            return 0;
        }
    }
    if (!bin_path) {
        fputs(usage_text, stdout);
        return 1;
    }
    if (n_batch > 1 && n_gpus > 1) {
        fprintf(stderr, "error: --batch and --gpus do not combine: shard groups are not batched\n");
        return 1;
    }
    if (score && (n_batch > 1 || n_gpus > 1)) {
        fprintf(stderr, "error: --score does not combine with %s: one sequence on one GPU is scored per run\n",
                n_batch > 1 ? "--batch" : "--gpus");
        return 1;
    }
    if (spec_sample >= 0 && (spec >= 0 || score || n_batch > 1 || n_gpus > 1)) {
        fprintf(stderr, "error: --spec-sample does not combine with %s: one sequence on one GPU is decoded per run%s\n",
                spec >= 0 ? "--spec" : score ? "--score" : n_batch > 1 ? "--batch" : "--gpus",
                spec >= 0 ? ", by one of the two loops" : "");
        return 1;
    }
    if (spec_sample >= 0 && !(std::isfinite(temperature) && temperature >= 0.0f)) {
        fprintf(stderr, "error: --spec-sample needs a temperature that is finite and >= 0 (it is %g)\n", temperature);
        return 1;
    }
    if (spec >= 0 && (score || n_batch > 1 || n_gpus > 1)) {
        fprintf(stderr, "error: --spec does not combine with %s: one sequence on one GPU is decoded per run\n",
                score ? "--score" : n_batch > 1 ? "--batch" : "--gpus");
        return 1;
    }
    if (spec >= 0 && temperature != 0.0f) {
        fprintf(stderr, "error: --spec is greedy decoding only: add -t 0 (the temperature is %g), or use --spec-sample\n",
                temperature);
        return 1;
    }

    // ---- ranks (before any GPU call: the children must start with a clean HIP state)
    std::string xdir;
    std::vector<pid_t> kids;
    if (n_gpus > 1) {
        setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0", 0);  // dmabuf IPC
        char tmpl[] = "/tmp/llama2_ranks_XXXXXX";
        if (!mkdtemp(tmpl)) {
            fprintf(stderr, "error: cannot create a temporary directory for the rank hand-shake\n");
            return 1;
        }
        xdir = tmpl;
        g_world = n_gpus;
        fflush(stdout);
        fflush(stderr);
        for (int r = 1; r < n_gpus; r++) {
            const pid_t pid = fork();
            if (pid < 0) {
                fprintf(stderr, "error: fork failed\n");
                return 1;
            }
            if (pid == 0) {
                g_rank = r;
                kids.clear();
                verbose = false;
                dump_tokens = false;
                break;
            }
            kids.push_back(pid);
        }
    }
    auto finish = [&](int rc) -> int {  // children leave quietly; rank 0 reaps them and cleans up
        fflush(stdout);
        if (g_rank != 0) _exit(rc);
        for (pid_t k : kids) {
            int st = 0;
            waitpid(k, &st, 0);
            if (rc == 0 && !(WIFEXITED(st) && WEXITSTATUS(st) == 0)) rc = 1;
        }
        if (!xdir.empty()) {
            for (int r = 0; r < g_world; r++) {
                unlink((xdir + "/h" + std::to_string(r)).c_str());
                unlink((xdir + "/e" + std::to_string(r)).c_str());
            }
            rmdir(xdir.c_str());
        }
        return rc;
    };

    // ---- checkpoint: 28-byte header + f32 blob (:936-967); mmap instead of a heap copy:
    // l2z_weights_init streams it to the GPU once and the mapping is dropped
    const int fd = open(bin_path, O_RDONLY);
    if (fd < 0) {
        if (g_rank == 0) fprintf(stderr, "error: cannot open checkpoint '%s'\n", bin_path);
        return finish(1);
    }
    struct stat st;
    if (fstat(fd, &st) != 0 || (size_t)st.st_size < sizeof(l2z_config)) {
        if (g_rank == 0) fprintf(stderr, "error: checkpoint '%s' is too small\n", bin_path);
        return finish(1);
    }
    void *map = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (map == MAP_FAILED) {
        if (g_rank == 0) fprintf(stderr, "error: mmap of '%s' failed\n", bin_path);
        return finish(1);
    }
    l2z_config cfg;
    memcpy(&cfg, map, sizeof cfg);                       // :941
    const bool shared_weights = cfg.vocab_size > 0;      // :943
    cfg.vocab_size = abs(cfg.vocab_size);                // :944
    LOGV("config: dim %d hidden_dim %d n_layers %d n_heads %d n_kv_heads %d vocab_size %d seq_len %d\n",
         cfg.dim, cfg.hidden_dim, cfg.n_layers, cfg.n_heads, cfg.n_kv_heads, cfg.vocab_size, cfg.seq_len);
    LOGV("shared weights: %s\ntemperature: %g\ntop-p: %g\n", shared_weights ? "true" : "false",
         temperature, top_p);
    int device = 0;
    {
        char name[256] = "";
        int cus = 0, n_dev = 0;
        uint64_t hbm = 0;
        if (l2z_device_count(&n_dev) != L2Z_OK || n_dev < 1) return finish(die("no GPU"));
        device = g_rank % n_dev;  // fewer GPUs than ranks: ranks share (functional, not fast)
        if (g_world > n_dev) {
            // Ranks sharing a chip: a mat-vec that polls for a peer's words must leave the peer's producer
            // room to run, else the waits time out (at most 512 polling blocks on the chip in
            // total).  The library reads its knobs once, at first use -- nothing has used them yet.
            const int per_dev = (g_world + n_dev - 1) / n_dev;
            const int cap = 512 / per_dev < 32 ? 32 : 512 / per_dev;
            setenv("L2Z_GRID_CAP", std::to_string(cap).c_str(), 0);
        }
        if (l2z_device_info(device, name, sizeof name, &cus, &hbm) != L2Z_OK) return finish(die("no GPU"));
        LOGV("device: %s, %d CUs, %.0f GB HBM%s\n\n", name, cus, (double)hbm / 1e9,
             g_world > 1 ? " (rank 0 of the shard group)" : "");
    }
    l2z_comm *comm = nullptr;
    if (g_world > 1) {
        if (l2z_comm_init(g_rank, g_world, nullptr, device, &comm) != L2Z_OK) {
            mark_failed(xdir);
            return finish(die("comm_init"));
        }
        char handle[L2Z_COMM_IPC_BYTES];
        // (world * dim: under L2Z_SCHEME_B every rank's whole partial [dim] vector lands in every slot)
        const size_t longest = std::max((size_t)std::max(std::max(cfg.dim, cfg.hidden_dim), cfg.vocab_size),
                                        (size_t)g_world * (size_t)cfg.dim);
        const size_t widest = (size_t)std::max(cfg.dim, cfg.hidden_dim);  // bulk regions: [chunk, dim | hidden_dim]
        std::vector<char> all;
        if (l2z_comm_p2p_export_sized(comm, longest, widest, handle) != L2Z_OK) {
            mark_failed(xdir);
            return finish(die("p2p_export"));
        }
        if (!exchange_handles(xdir, kids, handle, &all)) {
            mark_failed(xdir);
            fprintf(stderr, "error: rank %d: hand-shake with the other ranks failed (a rank could not set up "
                            "its GPU, or died)\n", g_rank);
            return finish(1);
        }
        if (l2z_comm_p2p_connect(comm, all.data()) != L2Z_OK) return finish(die("p2p_connect"));
    }
    const float *data = reinterpret_cast<const float *>(static_cast<const char *>(map) + sizeof cfg);
    const size_t n_floats = ((size_t)st.st_size - sizeof cfg) / sizeof(float);
    l2z_weights *w = nullptr;
    const auto t_up = std::chrono::steady_clock::now();
    if (l2z_weights_init(&cfg, data, n_floats, shared_weights, comm, &w) != L2Z_OK)
        return finish(die("Weights.init"));
    {
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_up).count();
        LOGV("weights: %.2f GB of the file%s on the GPU in %.2f s\n", (double)st.st_size / 1e9 / g_world,
             g_world > 1 ? " (this rank's rows)" : "", el);
    }
    munmap(map, (size_t)st.st_size);
    close(fd);

    Tokenizer tok;  // :970
    std::string err;
    if (!tok.from_file(tokenizer_path, (size_t)cfg.vocab_size, &err)) {
        if (g_rank == 0) fprintf(stderr, "error: %s\n", err.c_str());
        return finish(1);
    }
    l2z_runstate *s = nullptr;  // :974
    if (l2z_runstate_init(&cfg, comm, &s) != L2Z_OK) return finish(die("RunState.init"));

    std::vector<int32_t> prompt;  // :978-985
    if (input && !tok.encode(input, &prompt, &err)) {
        if (g_rank == 0) fprintf(stderr, "error: cannot encode the prompt: %s\n", err.c_str());
        return finish(1);
    }
    const size_t prompt_len = prompt.size();
    if (score) {
        const int rc = run_score(cfg, w, s, tok, prompt);
        l2z_runstate_free(s);
        l2z_weights_free(w);
        return finish(rc);
    }

    seq_len = seq_len == 0 ? (size_t)cfg.seq_len : seq_len;                        // :992
    seq_len = seq_len < 1 ? 1 : (seq_len > (size_t)cfg.seq_len ? (size_t)cfg.seq_len : seq_len);  // :993

    if (spec >= 0 || spec_sample >= 0) {
        const SpecDraw draw = {temperature, top_p, &prng};
        const int rc = run_spec(spec >= 0 ? spec : spec_sample, cfg, w, s, tok, prompt, seq_len, dump_tokens,
                                spec_sample >= 0 ? &draw : nullptr);
        l2z_runstate_free(s);
        l2z_weights_free(w);
        return finish(rc);
    }
    if (n_batch > 1) {
        const int rc = run_batch(n_batch, cfg, w, s, tok, prompt, seq_len, temperature, top_p, seed, dump_tokens);
        l2z_runstate_free(s);
        l2z_weights_free(w);
        return finish(rc);
    }

    std::vector<float> logits((size_t)cfg.vocab_size);
    std::vector<IndexedF32> logits_indexed;
    std::vector<int32_t> produced;
    bool timer_started = false;
    std::chrono::steady_clock::time_point t0;
    size_t token = 1, pos = 0;  // :988, :994

    // print one token exactly as :1022-1041 does; returns false if the sequence ended
    auto emit = [&](size_t next) -> bool {
        produced.push_back((int32_t)next);
        if (next == 1) return false;  // :1017
        std::string_view piece = tok.tokens[next];
        if (token == 1 && !piece.empty() && piece[0] == ' ') piece.remove_prefix(1);  // :1022-1025
        const int byte = is_raw_byte(piece);
        if (byte >= 0) {  // :1028-1031: printed, but the timer is not started on this path
            if (g_rank == 0) fputc(byte, stdout);
            token = next;
            return true;
        }
        if (g_rank == 0) fwrite(piece.data(), 1, piece.size(), stdout);
        token = next;
        if (!timer_started) {  // :1039-1041
            fflush(stdout);
            timer_started = true;
            t0 = std::chrono::steady_clock::now();
        }
        return true;
    };

    if (temperature == 0.0f) {
        // the loop of :995-1042 on the device; prompt override included
        if (l2z_greedy_begin(s, prompt.data(), (int)prompt_len) != L2Z_OK) return finish(die("greedy_begin"));
        std::vector<int32_t> chunk(64);
        bool alive = true;
        // tokens per call: the text appears in bursts of one call, so keep a call near 40 ms -- 64 tokens for
        // the small models, ~9 for the 7B shape (a call costs one stream synchronisation, ~20 us)
        size_t step = 8;
        if (g_world > 1) {
            // The ranks share no control plane: they stay in step only because every rank makes the SAME
            // sequence of calls.  A step sized from this rank's own clock can differ between ranks (9 vs 8
            // tokens), and when a BOS then ends the sequence inside a call the rank that asked for more has
            // queued passes its peers never run (a 20 s gather timeout, stores into a freed arena).  So the
            // step is a function of the model and the rank count only: this rank's weight bytes per token at
            // ~5 TB/s plus ~5 us per gather, sized for the same ~40 ms bursts.
            const double wbytes = 4.0 * ((double)cfg.n_layers * (2.0 * cfg.dim * cfg.dim +
                                                                2.0 * cfg.dim * (cfg.dim / cfg.n_heads) * cfg.n_kv_heads +
                                                                3.0 * cfg.dim * cfg.hidden_dim) +
                                         (double)cfg.vocab_size * cfg.dim) / g_world;
            const double per = wbytes / 5.0e12 + (4.0 * cfg.n_layers + 1.0) * 5.0e-6;
            const double fit = 0.040 / per;
            step = fit < 4.0 ? 4 : fit > 64.0 ? 64 : (size_t)fit;
        }
        while (alive && pos < seq_len) {
            // first token alone so the clock starts where the reference starts it; a prompt of
            // L2Z_PREFILL_MIN_PROMPT tokens or more is asked for in one call so that the library
            // runs its positions as one batched pass (they then print in a burst)
            int want = pos == 0 ? 1 : (int)std::min<size_t>(step, seq_len - pos);
            if (pos == 0 && prompt_len >= L2Z_PREFILL_MIN_PROMPT && prompt_len <= seq_len) {
                want = (int)prompt_len;
                chunk.resize(std::max(chunk.size(), prompt_len));
            }
            int got = 0;
            const auto tc = std::chrono::steady_clock::now();
            if (l2z_greedy_run(&cfg, s, w, want, chunk.data(), &got) != L2Z_OK) return finish(die("greedy_run"));
            if (got == 0) break;
            if (g_world == 1 && pos > 0 && got == want && want >= 4) {
                const double per = std::chrono::duration<double>(std::chrono::steady_clock::now() - tc).count() / got;
                const double fit = per > 0.0 ? 0.040 / per : 64.0;
                step = fit < 4.0 ? 4 : fit > 64.0 ? 64 : (size_t)fit;
            }
            for (int i = 0; i < got && alive; i++) {
                alive = emit((size_t)chunk[(size_t)i]);
                if (alive) pos++;
            }
        }
    } else {
        // The prompt positions (:999-1000: next = prompt[pos], their logits are never sampled) as
        // one batched pass when the prompt is long enough; the tokens print in a burst, then the
        // loop continues at pos = prompt_len.  Any refusal (odd dims, L2Z_PREFILL=0, a BOS inside
        // the prompt, which would end the loop at :1017) leaves the stepped loop below to do it.
        // L2Z_HOST_SOFTMAX=1: divide + softmax on the host in the reference's order (:1005-1008) instead of
        // l2z_probs_read -- the device reduces the denominator as a tree, so probabilities can differ in the
        // last ulp and a fixed seed can (rarely) land on the other side of a cdf boundary
        const char *hs_env = getenv("L2Z_HOST_SOFTMAX");
        const bool host_softmax = hs_env && atoi(hs_env) != 0;
        const char *pf_env = getenv("L2Z_PREFILL");
        bool has_bos = false;
        for (int32_t t : prompt) has_bos = has_bos || t == 1;
        if (prompt_len >= L2Z_PREFILL_MIN_PROMPT && prompt_len <= seq_len && !has_bos &&
            !(pf_env && atoi(pf_env) == 0)) {  // (a shard group without a bulk transport refuses: stepped loop)
            std::vector<int32_t> in(prompt_len);
            in[0] = 1;
            for (size_t i = 1; i < prompt_len; i++) in[i] = prompt[i - 1];
            if (l2z_prefill(in.data(), (int)prompt_len, 0, &cfg, s, w) == L2Z_OK) {
                for (size_t i = 0; i < prompt_len; i++) emit((size_t)prompt[i]);
                pos = prompt_len;
            }
        }
        for (; pos < seq_len; pos++) {
            if (l2z_transformer((int)token, (int)pos, &cfg, s, w) != L2Z_OK) return finish(die("transformer"));  // :996
            size_t next;
            if (pos < prompt_len) {
                next = (size_t)prompt[pos];  // :999-1000
            } else {
                // :1005-1008 (logits / temperature, softmax) on the device, then the copy the samplers need
                // anyway: 32000 exp() on one host core take as long as a small model's forward pass
                if (host_softmax) {
                    if (l2z_logits_read(s, logits.data()) != L2Z_OK) return finish(die("logits_read"));
                    for (float &v : logits) v /= temperature;  // :1006
                    softmax(logits.data(), logits.size());      // :1008
                } else if (l2z_probs_read(s, temperature, logits.data()) != L2Z_OK) {
                    return finish(die("probs_read"));
                }
                next = (top_p == 0.0f || top_p == 1.0f)         // :1009-1012
                           ? sample(logits.data(), logits.size(), prng)
                           : sample_top_p(logits.data(), logits.size(), top_p, logits_indexed, prng);
            }
            if (!emit(next)) break;
        }
    }
    fflush(stdout);
    if (timer_started) {  // :1043-1050 (the reference panics when no token was ever printed)
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const double tps = pos >= 1 ? (double)(pos - 1) / el : 0.0;
        LOGV("\n\n%u tokens per second\n", (unsigned)tps);
    }
    if (dump_tokens) {
        fprintf(stderr, "tokens:");
        for (int32_t t : produced) fprintf(stderr, " %d", t);
        fprintf(stderr, "\n");
    }
    l2z_runstate_free(s);
    l2z_weights_free(w);
    if (comm) l2z_comm_free(comm);
    return finish(0);
}
