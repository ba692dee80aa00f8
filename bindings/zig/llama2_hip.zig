//! llama2_hip.zig -- Zig declarations for include/llama2_hip.h (ABI version 2).
//!
//! Drop this file next to the reference's src/main.zig; main_hip.patch makes
//! main() call through it and build_hip.patch links libllama2_hip.so.
//!
//! Each extern replaces one site of the reference (cgbur/llama2.zig, src/main.zig):
//!   ConfigReader :17-25          L2zConfig (same 7 x i32, extern layout)
//!   Weights.init :73, :967       l2z_weights_init
//!   RunState.init :137, :974     l2z_runstate_init
//!   RunState.deinit :156, :975   l2z_runstate_free / l2z_weights_free
//!   transformer :285, :996       l2z_transformer
//!   argmax :715, :1003           l2z_argmax
//!   state.logits :1005-1012      l2z_logits_read / l2z_probs_read
//!   the -t 0 loop :995-1042      l2z_greedy_begin / l2z_greedy_run (optional fast path)
//!   prompt positions :999-1000   l2z_prefill (optional)
//!
//! Written against Zig 0.16 (build.zig.zon:5 of the reference).  The build
//! image of this repository has no Zig compiler: tests/test_zig_shim.py builds
//! and runs this file wherever `zig version` reports 0.16 and skips otherwise.
const std = @import("std");

pub const abi_version: c_int = 2;

/// == ConfigReader (main.zig:17-25) after :944 made vocab_size positive.
pub const L2zConfig = extern struct {
    dim: i32,
    hidden_dim: i32,
    n_layers: i32,
    n_heads: i32,
    n_kv_heads: i32,
    vocab_size: i32,
    seq_len: i32,
};

comptime {
    std.debug.assert(@sizeOf(L2zConfig) == 28);
    std.debug.assert(@offsetOf(L2zConfig, "seq_len") == 24);
}

pub const L2zWeights = opaque {};
pub const L2zRunState = opaque {};
pub const L2zComm = opaque {};

/// l2z_status of include/llama2_hip.h
pub const Status = enum(c_int) {
    ok = 0,
    invalid = -1,
    no_device = -2,
    hip = -3,
    oom = -4,
    comm = -5,
    state = -6,
    _,
};

pub extern fn l2z_abi_version() c_int;
pub extern fn l2z_last_error() [*:0]const u8;
pub extern fn l2z_device_count(out_n: *c_int) c_int;

pub extern fn l2z_weights_init(
    config: *const L2zConfig,
    data: [*]const f32,
    n_floats: usize,
    shared_weights: c_int,
    comm: ?*const L2zComm,
    out: *?*L2zWeights,
) c_int;
pub extern fn l2z_weights_free(w: ?*L2zWeights) void;

pub extern fn l2z_runstate_init(config: *const L2zConfig, comm: ?*const L2zComm, out: *?*L2zRunState) c_int;
pub extern fn l2z_runstate_free(s: ?*L2zRunState) void;

pub extern fn l2z_transformer(
    token: c_int,
    pos: c_int,
    config: *const L2zConfig,
    s: *L2zRunState,
    w: *const L2zWeights,
) c_int;
pub extern fn l2z_argmax(s: *L2zRunState, out_token: *c_int) c_int;
pub extern fn l2z_logits_read(s: *L2zRunState, out_logits: [*]f32) c_int;
pub extern fn l2z_probs_read(s: *L2zRunState, temperature: f32, out_probs: [*]f32) c_int;

pub extern fn l2z_greedy_begin(s: *L2zRunState, prompt: ?[*]const i32, n_prompt: c_int) c_int;
pub extern fn l2z_greedy_run(
    config: *const L2zConfig,
    s: *L2zRunState,
    w: *const L2zWeights,
    n_steps: c_int,
    out_tokens: [*]i32,
    out_n: *c_int,
) c_int;
pub extern fn l2z_prefill(
    tokens: [*]const i32,
    n_tokens: c_int,
    pos0: c_int,
    config: *const L2zConfig,
    s: *L2zRunState,
    w: *const L2zWeights,
) c_int;
/// l2z_prefill's state change plus, per position, the log-prob of targets[i] (-1: none -> 0) and the top-1 token id (no
/// reference equivalent).  out_logprob is null iff targets is; out_top1 may be null; not both.
pub extern fn l2z_score(
    tokens: [*]const i32,
    n_tokens: c_int,
    pos0: c_int,
    targets: ?[*]const i32,
    config: *const L2zConfig,
    s: *L2zRunState,
    w: *const L2zWeights,
    out_logprob: ?[*]f32,
    out_top1: ?[*]i32,
) c_int;
/// Speculative greedy decoding (no reference equivalent): tokens[0] is the sequence's token at pos0, tokens[1 ..] are
/// guesses for the positions after it; one sweep of the weights.  out_next[i] = the model's argmax after tokens[0 .. i],
/// out_accepted = a = how many leading guesses it agrees with; out_next[0 .. a] are the sequence's next a + 1 tokens and
/// the next position is pos0 + a + 1.  The ids a greedy loop emits do not depend on the guesses.
pub extern fn l2z_verify(
    tokens: [*]const i32,
    n_tokens: c_int,
    pos0: c_int,
    config: *const L2zConfig,
    s: *L2zRunState,
    w: *const L2zWeights,
    out_next: [*]i32,
    out_accepted: *c_int,
) c_int;
/// Speculative decoding under the sampler (no reference equivalent): l2z_verify with out_next[i] = the token
/// l2z_sample_batch draws from row i's logits with (temperature, top_p, coins[i]); coins[i] is the number of position
/// pos0 + i (one std.Random.float(f32) per generated token, kept when its row is rejected and passed again).  A guess is
/// accepted when it is the token drawn.  temperature 0: l2z_verify, coins may be null.
pub extern fn l2z_verify_sample(
    tokens: [*]const i32,
    n_tokens: c_int,
    pos0: c_int,
    temperature: f32,
    top_p: f32,
    coins: ?[*]const f32,
    config: *const L2zConfig,
    s: *L2zRunState,
    w: *const L2zWeights,
    out_next: [*]i32,
    out_accepted: *c_int,
) c_int;
pub extern fn l2z_synchronize(s: *L2zRunState) c_int;
/// Batched decode (no reference equivalent): up to batch_max sequences, one runstate each, one token each, one sweep
/// of the weights -- the state change of l2z_transformer(tokens[i], pos[i], config, states[i], w) for every i.
pub const batch_max: c_int = 16;
pub extern fn l2z_transformer_batch(
    n: c_int,
    tokens: [*]const i32,
    pos: [*]const i32,
    config: *const L2zConfig,
    states: [*]const *L2zRunState,
    w: *const L2zWeights,
) c_int;
pub extern fn l2z_argmax_batch(n: c_int, states: [*]const *L2zRunState, out_tokens: [*]i32) c_int;
/// main.zig:1002-1012 for n runstates on the device: the token the host samplers draw from states[i]'s logits with
/// temperature[i], top_p[i] and the drawn number coins[i] (one std.Random.float(f32) per sampled token).
pub extern fn l2z_sample_batch(
    n: c_int,
    states: [*]const *L2zRunState,
    temperature: [*]const f32,
    top_p: [*]const f32,
    coins: [*]const f32,
    out_tokens: [*]i32,
) c_int;
/// dst takes src's KV-cache rows 0 .. n_pos-1 and its logits; dst's next position is n_pos (one prompt, many samples).
pub extern fn l2z_runstate_fork(dst: *L2zRunState, src: *const L2zRunState, n_pos: c_int) c_int;

pub const Error = error{DeviceForwardFailed};

/// The reference's transformer() cannot fail; a device path can.  Every entry
/// point returns 0 or a negative l2z_status: print the library's message and
/// turn it into a Zig error.
pub fn check(rc: c_int) Error!void {
    if (rc != 0) {
        std.debug.print("llama2_hip: {s} (status {d})\n", .{ l2z_last_error(), rc });
        return error.DeviceForwardFailed;
    }
}

/// Device-side twins of the reference's Weights + RunState, made once after
/// the checkpoint is in memory (main.zig:967, :974) and freed with deinit().
pub const Device = struct {
    cfg: L2zConfig,
    w: *L2zWeights,
    s: *L2zRunState,

    /// `data` is the blob that follows the 28-byte header (main.zig:957-965);
    /// it may be freed as soon as this returns.
    pub fn init(cfg: L2zConfig, data: []align(4) const u8, shared_weights: bool) Error!Device {
        if (l2z_abi_version() != abi_version) {
            std.debug.print("llama2_hip: library ABI {d}, binding ABI {d}\n", .{ l2z_abi_version(), abi_version });
            return error.DeviceForwardFailed;
        }
        var w: ?*L2zWeights = null;
        try check(l2z_weights_init(&cfg, @ptrCast(data.ptr), data.len / 4, @intFromBool(shared_weights), null, &w));
        errdefer l2z_weights_free(w);
        var s: ?*L2zRunState = null;
        try check(l2z_runstate_init(&cfg, null, &s));
        return .{ .cfg = cfg, .w = w.?, .s = s.? };
    }

    pub fn deinit(self: *Device) void {
        l2z_runstate_free(self.s);
        l2z_weights_free(self.w);
        self.* = undefined;
    }

    /// main.zig:996
    pub fn transformer(self: *Device, token: usize, pos: usize) Error!void {
        try check(l2z_transformer(@intCast(token), @intCast(pos), &self.cfg, self.s, self.w));
    }

    /// main.zig:1003 -- on the device, strict '>' (lowest index wins ties, :720)
    pub fn argmax(self: *Device) Error!usize {
        var t: c_int = 0;
        try check(l2z_argmax(self.s, &t));
        return @intCast(t);
    }

    /// state.logits for the host samplers (main.zig:1005-1012)
    pub fn readLogits(self: *Device, logits: []f32) Error!void {
        std.debug.assert(logits.len == @as(usize, @intCast(self.cfg.vocab_size)));
        try check(l2z_logits_read(self.s, logits.ptr));
    }
};
