"""Single-env gym.Env adapter: step() latency (host attributes pushed, one env stepped on the GPU, state pulled back).
--wrap lidar | agentmap: the same loop through LidarInFront(env) / AgentMap(env), the reference's tests/random_action.py shape - every
step() then also computes an observation on the device."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import gym_novel_gridworlds_amd as G
ap = argparse.ArgumentParser()
ap.add_argument('--wrap', choices=('none', 'lidar', 'agentmap'), default='none')
ap.add_argument('--steps', type=int, default=2000)
args = ap.parse_args()
env = G.make('NovelGridworld-Pogostick-v1')
if args.wrap == 'lidar':
    env = G.LidarInFront(env, num_beams=8)
elif args.wrap == 'agentmap':
    env = G.AgentMap(env)
env.reset()
rs = np.random.RandomState(0)
acts = rs.randint(0, 17, size=args.steps)
for a in acts[:200]: env.step(int(a))
t = time.perf_counter()
for a in acts: env.step(int(a))
dt = time.perf_counter() - t
label = 'adapter step()' if args.wrap == 'none' else 'adapter + %s step()' % ('LidarInFront' if args.wrap == 'lidar' else 'AgentMap')
print('%s %.1f us -> %.0f env-steps/s' % (label, dt / len(acts) * 1e6, len(acts) / dt))
t = time.perf_counter()
for i in range(200): env.reset()
print('%s %.1f us' % (label.replace('step()', 'reset()'), (time.perf_counter() - t) / 200 * 1e6))
if args.wrap == 'none':
    vec = env._backend()
    t = time.perf_counter()
    for a in acts: vec.step1(int(a))
    print('  of which the C-ABI call (ngw_step_host through ctypes) %.1f us' % ((time.perf_counter() - t) / len(acts) * 1e6))
